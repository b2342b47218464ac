"""unmore_amd.box_loss on the MI355X: one ragged batch through match_and_label, fast_rcnn_losses / droploss_weights and
next_stage_proposals against the restatement of tests/box_loss_common.py, and the fixture of the reference's own box branch
(tests/golden/box_loss.npz) on the device, call by call and chained over its three stages."""
import numpy as np
import pytest
import torch

from box_loss_common import (STAGE_IOUS, STAGE_WEIGHTS, apply_deltas_np, clip_np, droploss_iou_max_np, droploss_weights_np, get_deltas_np,
                             load_fixture, logged_scalars, losses_reference, match_np, next_stage_np, ragged_batch)

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
W4 = STAGE_WEIGHTS[0]
THRESH, DROP = 0.5, 0.01
SINGLE = [0, 0, 1, 0, 0]


def _dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def batch():
    """Proposals per image 0, 1, 3, 65, 300 (a wavefront and a 256-thread workgroup are crossed); ground truths 5, 0, 1, GT_TILE + 1, 5
    (GT_TILE = the kernel's LDS tile of ground truths); frames of different sizes; small boxes, so that drop-loss drops a fair share."""
    from unmore_amd.box_loss import GT_TILE
    assert GT_TILE == 256
    sizes = [(48, 130), (60, 90), (37, 53), (48, 130), (64, 100)]
    images = ragged_batch(7, [0, 1, 3, 65, 300], [5, 0, 1, GT_TILE + 1, 5], sizes, box_scale=0.3)
    p, g = images[4]["proposal_boxes"], images[4]["gt_boxes"]
    p[10] = g[2]                                                  # an exact duplicate of a ground truth
    p[11] = [g[2][2], g[2][1], g[2][2] + 5, g[2][3]]              # touching it
    p[12] = [20, 10, 20, 30]                                      # zero area
    p[13] = [40, 10, 30, 30]                                      # negative width
    p[14] = [150, 80, 170, 95]                                    # outside the frame
    p[15] = [10, np.nan, 30, 30]                                  # the one bad row
    images[3]["gt_boxes"][7] = images[3]["gt_boxes"][3]           # duplicated ground truths: the tie goes to index 3
    images[3]["proposal_boxes"][5] = images[3]["gt_boxes"][3]
    images[3]["proposal_boxes"][6] = images[3]["gt_boxes"][GT_TILE]    # a copy of the one ground truth in the second LDS tile
    rng = np.random.RandomState(11)
    R = sum(len(im["proposal_boxes"]) for im in images)
    scores = (rng.standard_normal((R, 2)) * 3).astype(np.float32)
    deltas = (rng.standard_normal((R, 4)) * np.array(W4) * 0.05).astype(np.float32)
    deltas[3::17, 2] = 6.0 * W4[2]                                # dw / ww = 6: past the clamp at log(1000 / 16) = 4.135
    deltas[5::19, 3] = 5.0 * W4[3]
    deltas[8::13, 0] = 40.0 * W4[0]                               # 40 widths to the right: clips to zero width
    return {"images": images, "sizes": sizes, "scores": scores, "deltas": deltas, "R": R}


@pytest.fixture(scope="module")
def device_run(batch):
    """every call once, shared by the tests below"""
    from unmore_amd import box_loss as B
    dev = _dev()
    props = [{"proposal_boxes": _t(im["proposal_boxes"], dev)} for im in batch["images"]]
    targets = [{k: _t(im[k], dev) for k in ("gt_boxes", "gt_classes", "gt_scores")} for im in batch["images"]]
    mstats = {}
    matched = B.match_and_label(props, targets, THRESH, 1, stats=mstats)
    scores, deltas = _t(batch["scores"], dev).requires_grad_(True), _t(batch["deltas"], dev).requires_grad_(True)
    single = torch.tensor(SINGLE, device=dev)
    lstats = {}
    losses = B.fast_rcnn_losses(scores, deltas, matched, box2box_weights=W4, droploss=(DROP, single), stats=lstats)
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    boxes, keep, counts = B.next_stage_proposals(deltas, matched, W4, batch["sizes"], training=True)
    torch.cuda.synchronize()
    return {"B": B, "dev": dev, "props": props, "targets": targets, "matched": matched, "mstats": mstats, "scores": scores, "deltas": deltas,
            "single": single, "losses": losses, "lstats": lstats, "boxes": boxes, "keep": keep, "counts": counts}


@pytest.fixture(scope="module")
def matched_np(batch):
    return [match_np(im["proposal_boxes"], im["gt_boxes"], im["gt_classes"], im["gt_scores"], THRESH, 1, np.float32) for im in batch["images"]]


def test_match_equals_the_float32_restatement(batch, device_run, matched_np):
    got, st = device_run["matched"], device_run["mstats"]
    for k, (g, m) in enumerate(zip(got, matched_np)):
        assert np.array_equal(g["matched_vals"].cpu().numpy().view(np.uint32), m["matched_vals"].view(np.uint32)), k      # bit for bit
        assert np.array_equal(g["matched_idxs"].cpu().numpy(), m["matched_idxs"]) and g["matched_idxs"].dtype == torch.int64
        assert g["mask_index"] is g["matched_idxs"]
        for key in ("gt_classes", "gt_boxes", "gt_scores"):
            assert np.array_equal(g[key].cpu().numpy(), m[key]), (k, key)
    assert st["num_fg"].dtype == torch.int32 and st["num_fg"].is_cuda
    assert st["num_fg"].tolist() == [m["num_fg"] for m in matched_np] and st["num_bg"].tolist() == [m["num_bg"] for m in matched_np]
    assert st["bad"].tolist() == [0, 0, 0, 0, 1]
    N = len(matched_np)
    s = st["scalars"]()
    assert s == {"num_fg_samples": sum(m["num_fg"] for m in matched_np) / N, "num_bg_samples": sum(m["num_bg"] for m in matched_np) / N, "bad": 1}
    # the batch has what it is meant to have
    m4, m3 = matched_np[4], matched_np[3]
    assert m4["matched_vals"][10] == 1.0 and m4["matched_vals"][11] == 0 and not m4["matched_vals"][12:16].any() and m4["labels"][10]
    assert m3["matched_idxs"][5] == 3 and m3["matched_vals"][5] == 1.0
    assert m3["matched_idxs"][6] == 256 and m3["matched_vals"][6] == 1.0                                       # past the first LDS tile
    assert not got[1]["gt_boxes"].any() and not got[1]["gt_scores"].any() and got[1]["gt_classes"].tolist() == [1]    # no ground truths
    assert sum(m["num_fg"] for m in matched_np) >= 30


def _decided_rows(deltas, boxes, sizes):
    """rows whose keep / drop decision float32 cannot get wrong: finite, and each float64 extent after the clip is more than
    4 ulp * max(|coordinate|, frame side) from 0, or 0 because both ends sit beyond the same border by more than that"""
    c64, _, _ = next_stage_np(deltas, boxes, W4, sizes, True, np.float64)
    out, at = [], 0
    for k, b64 in enumerate(c64):
        n = len(b64)
        pre = apply_deltas_np(deltas[at:at + n], boxes[k], W4, np.float64)
        bound = 4 * EPS32 * np.maximum(np.abs(b64), max(sizes[k]))
        decided = np.isfinite(b64).all(axis=1)
        for lo, hi, lim in ((0, 2, sizes[k][1]), (1, 3, sizes[k][0])):
            ext, b = b64[:, hi] - b64[:, lo], np.maximum(bound[:, lo], bound[:, hi])
            pinned = ((pre[:, lo] > lim + b) & (pre[:, hi] > lim + b)) | ((pre[:, lo] < -b) & (pre[:, hi] < -b))
            decided &= (np.abs(ext) > b) | pinned
        out.append(decided)
        at += n
    return np.concatenate(out)


def test_decode_clip_and_compaction(batch, device_run):
    ims, sizes = batch["images"], batch["sizes"]
    boxes = [im["proposal_boxes"] for im in ims]
    c64, _, _ = next_stage_np(batch["deltas"], boxes, W4, sizes, True, np.float64)
    c32, keep32, _ = next_stage_np(batch["deltas"], boxes, W4, sizes, True, np.float32)
    keep, counts = device_run["keep"].cpu().numpy(), device_run["counts"].cpu().numpy()
    out = device_run["boxes"].cpu().numpy()
    assert counts.dtype == np.int32 and keep.dtype == bool
    at, dst, worst, undecided = 0, 0, 0.0, 0
    for k, (b64, b32) in enumerate(zip(c64, c32)):
        n, side = len(b64), max(sizes[k])
        kk = keep[at:at + n]
        assert counts[k] == kk.sum()
        got = out[dst:dst + counts[k]]                                         # compacted in order, image after image
        finite = np.isfinite(b64).all(axis=1)
        bound = 4 * EPS32 * np.maximum(np.abs(b64), side)
        err = np.abs(got - b64[kk])
        ok = finite[kk]
        worst = max(worst, float((err[ok] / bound[kk][ok]).max()) if ok.any() else 0.0)
        assert (err[ok] <= bound[kk][ok]).all(), k
        # a row is decided when both float64 extents are more than the bound from 0, or 0 because both ends sit on the same border
        pre = apply_deltas_np(batch["deltas"][at:at + n], boxes[k], W4, np.float64)
        decided = np.ones(n, dtype=bool)
        for lo, hi, lim in ((0, 2, sizes[k][1]), (1, 3, sizes[k][0])):
            ext, b = b64[:, hi] - b64[:, lo], np.maximum(bound[:, lo], bound[:, hi])
            pinned = ((pre[:, lo] > lim + b) & (pre[:, hi] > lim + b)) | ((pre[:, lo] < -b) & (pre[:, hi] < -b))
            decided &= (np.abs(ext) > b) | pinned
        decided &= finite
        undecided += int((~decided & finite).sum())
        assert np.array_equal(kk[decided], keep32[at:at + n][decided]), k
        assert not kk[~finite].any()
        at, dst = at + n, dst + counts[k]
    print(f"decode: worst error {worst:.3f} of the bound 4 ulp * max(|coordinate|, frame side); {undecided} undecided rows")
    assert undecided <= 0.01 * batch["R"]
    assert 0.05 * batch["R"] < (~keep).sum() < 0.5 * batch["R"]                 # boxes were dropped, most were kept
    # at inference nothing is dropped
    B = device_run["B"]
    b_inf, k_inf, c_inf = B.next_stage_proposals(device_run["deltas"], device_run["matched"], W4, sizes, training=False)
    assert k_inf.all() and c_inf.tolist() == [len(b) for b in boxes]
    flat64 = np.concatenate(c64)
    fin = np.isfinite(flat64)
    assert (np.abs(b_inf.cpu().numpy() - flat64)[fin] <= (4 * EPS32 * np.maximum(np.abs(flat64), 130))[fin]).all()
    parts = B.split_proposals(device_run["boxes"], device_run["counts"])
    assert [len(p) for p in parts] == counts.tolist()
    # the plain ops
    flat = _t(np.concatenate(boxes), device_run["dev"])
    ap = B.apply_deltas(device_run["deltas"], flat, W4).cpu().numpy()
    p64 = apply_deltas_np(batch["deltas"], np.concatenate(boxes), W4, np.float64)
    fin = np.isfinite(p64)
    assert (np.abs(ap - p64)[fin] <= (4 * EPS32 * np.maximum(np.abs(p64), 130 * 63))[fin]).all()     # unclipped: up to 62.5 box widths
    gtb = torch.cat([m["gt_boxes"] for m in device_run["matched"]])
    gd = B.get_deltas(flat, gtb, W4).cpu().numpy()
    src = np.concatenate(boxes).astype(np.float64)
    g64 = get_deltas_np(src, gtb.cpu().numpy(), W4, np.float64)
    fin = np.isfinite(g64).all(axis=1) & np.isfinite(gd).all(axis=1) & (src[:, 2] - src[:, 0] > 0.5) & (src[:, 3] - src[:, 1] > 0.5)
    # the centres are rounded at the frame's scale (130) before they are subtracted and divided by the source extent
    extent = np.minimum(src[:, 2] - src[:, 0], src[:, 3] - src[:, 1])[fin, None]
    assert fin.sum() > 300 and (np.abs(gd[fin] - g64[fin]) <= 1e-5 * np.abs(g64[fin]) + W4[0] * 8 * EPS32 * 130 / extent).all()


def test_drop_weights(batch, device_run, matched_np):
    w = device_run["lstats"]["weights"].cpu().numpy()
    boxes = [im["proposal_boxes"] for im in batch["images"]]
    iou64 = droploss_iou_max_np(batch["deltas"], boxes, [m["gt_boxes"] for m in matched_np], W4, np.float64)
    want = droploss_weights_np(iou64, DROP, SINGLE, len(boxes))
    decided = ~(np.abs(iou64 - DROP) <= 1e-5) | np.isnan(iou64)
    R = batch["R"]
    per = R // len(boxes)
    decided |= (np.arange(R) // per < len(boxes)) & (np.array(SINGLE + [0])[np.minimum(np.arange(R) // per, len(boxes))] == 1)
    assert np.array_equal(w[decided], want[decided])
    assert (~decided).sum() <= 0.01 * R
    assert (w == 0).sum() >= 0.1 * R and (w == 1).sum() >= 0.1 * R, ((w == 0).sum(), R)
    # the single-object indicator goes by position: rows [2 * per, 3 * per) whatever image they are in
    assert (w[2 * per:3 * per] == 1).all() and per == 73 and R % len(boxes) != 0
    # alone, and through weights=
    B = device_run["B"]
    alone = B.droploss_weights(device_run["deltas"], device_run["matched"], W4, DROP, device_run["single"])
    assert torch.equal(alone, device_run["lstats"]["weights"])
    s2, d2 = device_run["scores"].detach().clone().requires_grad_(True), device_run["deltas"].detach().clone().requires_grad_(True)
    st = {}
    again = B.fast_rcnn_losses(s2, d2, device_run["matched"], box2box_weights=W4, weights=alone, stats=st)
    (again["loss_cls"] + again["loss_box_reg"]).backward()
    for key in ("loss_cls", "loss_box_reg"):
        assert torch.equal(again[key], device_run["losses"][key])
    assert torch.equal(s2.grad, device_run["scores"].grad) and torch.equal(d2.grad, device_run["deltas"].grad)
    assert torch.equal(st["counters"], device_run["lstats"]["counters"]) and torch.equal(st["weights"], alone)


def _flat(matched_np, batch):
    return (np.concatenate([im["proposal_boxes"] for im in batch["images"]]), np.concatenate([m["gt_boxes"] for m in matched_np]),
            np.concatenate([m["gt_classes"] for m in matched_np]), np.concatenate([m["gt_scores"] for m in matched_np]))


def test_losses_gradients_and_counters(batch, device_run, matched_np):
    pb, gb, gc, gs = _flat(matched_np, batch)
    w = device_run["lstats"]["weights"].cpu().numpy()
    lc, lb, g_s, g_d, counters = losses_reference(batch["scores"], batch["deltas"], pb, gb, gc, gs, w, W4)
    R = batch["R"]
    got_c, got_b = float(device_run["losses"]["loss_cls"].detach()), float(device_run["losses"]["loss_box_reg"].detach())
    print(f"loss_cls {got_c!r} (float64 {lc!r}), loss_box_reg {got_b!r} (float64 {lb!r})")
    assert abs(got_c - lc) <= 1e-5 * max(1, abs(lc)) and abs(got_b - lb) <= 1e-5 * max(1, abs(lb))
    assert device_run["losses"]["loss_cls"].dtype == torch.float32 and device_run["losses"]["loss_cls"].dim() == 0
    for got, ref in ((device_run["scores"].grad, g_s), (device_run["deltas"].grad, g_d)):
        assert (np.abs(got.cpu().numpy() - ref) <= 1e-5 * np.abs(ref) + 1e-6 / R).all()
    assert np.abs(g_d).max() > 0 and (gs[gc == 0] == 0).any() and (gs[gc == 0] == 1).any()           # scores of 0 and 1 on foreground rows
    assert device_run["lstats"]["counters"].dtype == torch.int64 and device_run["lstats"]["counters"].tolist() == counters
    assert counters[0] == R and counters[1] >= 30 and counters[5] == (w == 0).sum() and counters[6] == 0
    s, want = device_run["lstats"]["scalars"](), logged_scalars(counters)
    assert set(want) == {"cls_accuracy", "fg_cls_accuracy", "false_negative"} and all(abs(s[k] - want[k]) <= 1e-12 for k in want)
    assert s["dropped"] == counters[5] and s["bad"] == 0


def test_bfloat16_inputs(batch, device_run, matched_np):
    B, dev = device_run["B"], device_run["dev"]
    pb, gb, gc, gs = _flat(matched_np, batch)
    s = _t(batch["scores"], dev).bfloat16().requires_grad_(True)
    d = _t(batch["deltas"], dev).bfloat16().requires_grad_(True)
    st = {}
    out = B.fast_rcnn_losses(s, d, device_run["matched"], box2box_weights=W4, droploss=(DROP, device_run["single"]), stats=st)
    (out["loss_cls"] + out["loss_box_reg"]).backward()
    assert s.grad.dtype == torch.bfloat16 and d.grad.dtype == torch.bfloat16 and out["loss_cls"].dtype == torch.float32
    s64, d64 = s.detach().double().cpu().numpy(), d.detach().double().cpu().numpy()
    lc, lb, g_s, g_d, counters = losses_reference(s64, d64, pb, gb, gc, gs, st["weights"].cpu().numpy(), W4)
    assert abs(float(out["loss_cls"].detach()) - lc) <= 1e-5 * max(1, abs(lc)) and abs(float(out["loss_box_reg"].detach()) - lb) <= 1e-5 * max(1, abs(lb))
    assert st["counters"].tolist() == counters
    for got, ref in ((s.grad, g_s), (d.grad, g_d)):
        got = got.double().cpu().numpy()
        ulp = np.where(ref != 0, 2.0 ** (np.floor(np.log2(np.abs(np.where(ref != 0, ref, 1.0)))) - 7), 0.0)    # one bfloat16 ulp of the float64 value
        assert (np.abs(got - ref) <= ulp).all(), float((np.abs(got - ref) / np.maximum(ulp, 1e-300)).max())
    # decode of the bfloat16 deltas: the float32 restatement on the rounded deltas, row by row on the decided rows
    b16, k16, c16 = B.next_stage_proposals(d, device_run["matched"], W4, batch["sizes"])
    boxes, d32 = [im["proposal_boxes"] for im in batch["images"]], d.detach().float().cpu().numpy()
    _, keep32, _ = next_stage_np(d32, boxes, W4, batch["sizes"], True, np.float32)
    decided = _decided_rows(d32, boxes, batch["sizes"])
    k16, c16 = k16.cpu().numpy(), c16.cpu().numpy()
    assert b16.dtype == torch.float32 and np.array_equal(k16[decided], keep32[decided]) and (~decided).sum() <= 0.01 * batch["R"]
    ends = np.cumsum([len(x) for x in boxes])
    assert c16.tolist() == [int(k16[e - len(x):e].sum()) for e, x in zip(ends, boxes)]


def test_backward_scales_each_gradient_by_its_own_scalar(device_run):
    B = device_run["B"]
    s, d = device_run["scores"].detach().clone().requires_grad_(True), device_run["deltas"].detach().clone().requires_grad_(True)
    out = B.fast_rcnn_losses(s, d, device_run["matched"], box2box_weights=W4, droploss=(DROP, device_run["single"]))
    (2 * out["loss_cls"] + 3 * out["loss_box_reg"]).backward()
    assert torch.equal(s.grad, device_run["scores"].grad * 2) and torch.equal(d.grad, device_run["deltas"].grad * 3)
    # loss_weight scales the outputs, and through them the gradients
    s2, d2 = s.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    out2 = B.fast_rcnn_losses(s2, d2, device_run["matched"], box2box_weights=W4, droploss=(DROP, device_run["single"]),
                              loss_weight={"loss_cls": 2.0, "loss_box_reg": 3.0})
    assert torch.equal(out2["loss_cls"], out["loss_cls"] * 2) and torch.equal(out2["loss_box_reg"], out["loss_box_reg"] * 3)
    (out2["loss_cls"] + out2["loss_box_reg"]).backward()
    assert torch.equal(s2.grad, s.grad) and torch.equal(d2.grad, d.grad)


def test_two_calls_give_the_same_bytes(batch, device_run):
    B = device_run["B"]
    st = {}
    matched = B.match_and_label(device_run["props"], device_run["targets"], THRESH, 1, stats=st)
    for a, b in zip(matched, device_run["matched"]):
        for key in ("matched_idxs", "gt_classes"):
            assert torch.equal(a[key], b[key])
        for key in ("matched_vals", "gt_boxes", "gt_scores"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32))
    assert torch.equal(st["counts"], device_run["mstats"]["counts"])
    s, d = device_run["scores"].detach().clone().requires_grad_(True), device_run["deltas"].detach().clone().requires_grad_(True)
    lst = {}
    out = B.fast_rcnn_losses(s, d, matched, box2box_weights=W4, droploss=(DROP, device_run["single"]), stats=lst)
    (out["loss_cls"] + out["loss_box_reg"]).backward()
    for key in ("loss_cls", "loss_box_reg"):
        assert torch.equal(out[key].view(torch.int32), device_run["losses"][key].view(torch.int32))
    assert torch.equal(s.grad.view(torch.int32), device_run["scores"].grad.view(torch.int32))
    assert torch.equal(d.grad.view(torch.int32), device_run["deltas"].grad.view(torch.int32))
    assert torch.equal(lst["counters"], device_run["lstats"]["counters"]) and torch.equal(lst["weights"], device_run["lstats"]["weights"])
    boxes, keep, counts = B.next_stage_proposals(d, matched, W4, batch["sizes"])
    n = int(counts.sum())
    assert torch.equal(keep, device_run["keep"]) and torch.equal(counts, device_run["counts"])
    assert torch.equal(boxes[:n].view(torch.int32), device_run["boxes"][:n].view(torch.int32))


def test_empty_and_background_only_batches(device_run):
    B, dev = device_run["B"], device_run["dev"]
    # R == 0
    s, d = torch.zeros(0, 2, device=dev, requires_grad=True), torch.zeros(0, 4, device=dev, requires_grad=True)
    empty = [{"proposal_boxes": torch.zeros(0, 4, device=dev), "gt_boxes": torch.zeros(0, 4, device=dev),
              "gt_classes": torch.zeros(0, dtype=torch.int64, device=dev), "gt_scores": torch.zeros(0, device=dev)}]
    st = {}
    out = B.fast_rcnn_losses(s, d, empty, box2box_weights=W4, droploss=(DROP, None), stats=st)
    assert float(out["loss_cls"]) == 0 and float(out["loss_box_reg"]) == 0 and out["loss_cls"].requires_grad and out["loss_box_reg"].requires_grad
    (out["loss_cls"] + out["loss_box_reg"]).backward()
    assert s.grad.shape == (0, 2) and d.grad.shape == (0, 4) and st["scalars"]() == {"dropped": 0, "bad": 0}
    m = B.match_and_label([torch.zeros(0, 4, device=dev)], [device_run["targets"][0]], 0.5)
    assert m[0]["matched_idxs"].shape == (0,) and m[0]["gt_boxes"].shape == (0, 4)
    b, k, c = B.next_stage_proposals(d, empty, W4, [(10, 10)])
    assert b.shape == (0, 4) and c.tolist() == [0]
    # no foreground row: image 1 has no ground truths
    props, targets = [device_run["props"][1]] * 3, [device_run["targets"][1]] * 3
    st = {}
    m = B.match_and_label(props, targets, 0.5, stats=st)
    assert st["num_fg"].tolist() == [0, 0, 0] and st["num_bg"].tolist() == [1, 1, 1]
    s = torch.tensor([[1.0, -1.0], [0.0, 0.0], [-2.0, 2.0]], device=dev, requires_grad=True)
    d = torch.ones(3, 4, device=dev, requires_grad=True)
    st = {}
    out = B.fast_rcnn_losses(s, d, m, box2box_weights=W4, stats=st)
    want = float(np.mean([np.log1p(np.exp(2.0)), np.log(2.0), np.log1p(np.exp(-4.0))]))       # every target is (0, 1)
    assert abs(float(out["loss_cls"]) - want) <= 1e-5 * max(1, want) and float(out["loss_box_reg"]) == 0
    (out["loss_cls"] + out["loss_box_reg"]).backward()
    assert not d.grad.any() and s.grad.abs().sum() > 0
    sc = st["scalars"]()
    assert set(sc) == {"cls_accuracy", "dropped", "bad"} and sc["cls_accuracy"] == 1 / 3 and (st["weights"] == 1).all()
    # a foreground row whose ground-truth extent is not positive adds no box term and is counted bad; hard targets with K = 3
    bad = [{"proposal_boxes": torch.tensor([[0., 0, 10, 10], [0, 0, 10, 10]], device=dev), "gt_boxes": torch.tensor([[5., 0, 5, 10], [1, 0, 11, 10]], device=dev),
            "gt_classes": torch.tensor([0, 2], device=dev), "gt_scores": torch.ones(2, device=dev)}]
    s3 = torch.zeros(2, 4, device=dev, requires_grad=True)
    d3 = torch.tensor([[1.0, 1, 1, 1], [3.0, 0, -2, 0]], device=dev, requires_grad=True)
    st = {}
    out = B.fast_rcnn_losses(s3, d3, bad, box2box_weights=W4, num_classes=3, use_soft_targets=False, smooth_l1_beta=1.0, stats=st)
    assert abs(float(out["loss_cls"]) - np.log(4)) <= 1e-5 * np.log(4)
    assert abs(float(out["loss_box_reg"]) - ((2 - 0.5) + 0 + (2 - 0.5) + 0) / 2) <= 1e-5                  # the second row: deltas (1, 0, 0, 0)
    (out["loss_cls"] + out["loss_box_reg"]).backward()
    assert d3.grad.tolist() == [[0, 0, 0, 0], [0.5, 0, -0.5, 0]] and st["counters"].tolist() == [2, 2, 1, 1, 0, 0, 1]
    assert torch.allclose(s3.grad, torch.tensor([[-0.375, 0.125, 0.125, 0.125], [0.125, 0.125, -0.375, 0.125]], device=dev), rtol=1e-6)


@pytest.fixture(scope="module")
def fixture_on_device():
    fx = load_fixture()
    dev = _dev()
    N = int(fx["n_images"])
    targets = [{k: _t(fx[f"im{i}_{k}"], dev) for k in ("gt_boxes", "gt_classes", "gt_scores")} for i in range(N)]
    return fx, dev, N, targets


def _check_stage_losses(fx, s, out, scores, deltas, weights, flat):
    lc, lb, g_s, g_d, _ = losses_reference(fx[f"st{s}_scores"], fx[f"st{s}_deltas"], flat[0], flat[1], flat[2], flat[3], weights, STAGE_WEIGHTS[s])
    R = len(flat[0])
    assert abs(float(out["loss_cls"]) - lc) <= 1e-5 * max(1, abs(lc)) and abs(float(out["loss_box_reg"]) - lb) <= 1e-5 * max(1, abs(lb)), s
    # ... which the fixture's own float32 values agree with (tests/test_box_loss_cpu.py ties them to float64 within 1e-6)
    assert abs(float(out["loss_cls"]) - fx[f"st{s}_loss_cls"]) <= 1.1e-5 * max(1, abs(lc))
    assert abs(float(out["loss_box_reg"]) - fx[f"st{s}_loss_box_reg"]) <= 1.1e-5 * max(1, abs(lb))
    assert (np.abs(scores.grad.cpu().numpy() - g_s) <= 1e-5 * np.abs(g_s) + 1e-6 / R).all()
    assert (np.abs(deltas.grad.cpu().numpy() - g_d) <= 1e-5 * np.abs(g_d) + 1e-6 / R).all()


def test_fixture_cases_on_the_device(fixture_on_device):
    from unmore_amd import box_loss as B
    fx, dev, N, targets = fixture_on_device
    single = _t(fx["single"], dev)
    sizes = [tuple(v) for v in fx["sizes"].tolist()]
    for s in range(3):
        props = [_t(fx[f"st{s}_im{k}_proposal_boxes"], dev) for k in range(N)]
        st = {}
        matched = B.match_and_label(props, targets, STAGE_IOUS[s], 1, stats=st)
        for k, m in enumerate(matched):
            assert np.array_equal(m["matched_idxs"].cpu().numpy(), fx[f"st{s}_im{k}_matched_idxs"])
            assert np.array_equal(m["matched_vals"].cpu().numpy().view(np.uint32), fx[f"st{s}_im{k}_matched_vals"].view(np.uint32))
            for key in ("gt_classes", "gt_boxes", "gt_scores"):
                assert np.array_equal(m[key].cpu().numpy(), fx[f"st{s}_im{k}_{key}"]), (s, k, key)
        sc = st["scalars"]()
        assert np.allclose([sc["num_fg_samples"], sc["num_bg_samples"]], fx[f"st{s}_num_fg_bg"], rtol=1e-12)
        scores, deltas = _t(fx[f"st{s}_scores"], dev).requires_grad_(True), _t(fx[f"st{s}_deltas"], dev).requires_grad_(True)
        lst = {}
        out = B.fast_rcnn_losses(scores, deltas, matched, box2box_weights=STAGE_WEIGHTS[s], droploss=(float(fx["drop_thresh"]), single), stats=lst)
        (out["loss_cls"] + out["loss_box_reg"]).backward()
        w = lst["weights"].cpu().numpy()
        boxes = [fx[f"st{s}_im{k}_proposal_boxes"] for k in range(N)]
        iou64 = droploss_iou_max_np(fx[f"st{s}_deltas"], boxes, [fx[f"st{s}_im{k}_gt_boxes"] for k in range(N)], STAGE_WEIGHTS[s], np.float64)
        decided = np.abs(iou64 - float(fx["drop_thresh"])) > 1e-5
        assert np.array_equal(w[decided], fx[f"st{s}_weights"][decided]) and decided.mean() >= 0.99
        flat = [np.concatenate([fx[f"st{s}_im{k}_{key}"] for k in range(N)]) for key in ("proposal_boxes", "gt_boxes", "gt_classes", "gt_scores")]
        _check_stage_losses(fx, s, out, scores, deltas, w, flat)
        got = lst["scalars"]()
        for key, v in zip(("cls_accuracy", "fg_cls_accuracy", "false_negative"), fx[f"st{s}_scalars"]):
            assert (key not in got) if np.isnan(v) else abs(got[key] - v) <= 1e-12
        if s == 0:                                                              # the variants: drop-loss off, hard targets with and without weights
            for name, soft, use_w in (("nodrop", True, False), ("hard_drop", False, True), ("hard_nodrop", False, False)):
                s2, d2 = scores.detach().clone().requires_grad_(True), deltas.detach().clone().requires_grad_(True)
                o = B.fast_rcnn_losses(s2, d2, matched, box2box_weights=STAGE_WEIGHTS[0], use_soft_targets=soft,
                                       weights=_t(fx["st0_weights"], dev) if use_w else None)
                (o["loss_cls"] + o["loss_box_reg"]).backward()
                # the same bounds as the stages: against the float64 restatement on the variant's own weights
                lc, lb, g_s, g_d, _ = losses_reference(fx["st0_scores"], fx["st0_deltas"], flat[0], flat[1], flat[2], flat[3],
                                                       fx["st0_weights"] if use_w else None, STAGE_WEIGHTS[0], use_soft_targets=soft)
                R = len(flat[0])
                for key, ref in (("loss_cls", lc), ("loss_box_reg", lb)):
                    assert abs(float(o[key].detach()) - ref) <= 1e-5 * max(1, abs(ref)), (name, key)
                for g, ref in ((s2.grad, g_s), (d2.grad, g_d)):
                    assert (np.abs(g.cpu().numpy() - ref) <= 1e-5 * np.abs(ref) + 1e-6 / R).all(), name
                # and, beside it, the fixture's own float32 numbers: 1e-5 plus the 1e-6 that tests/test_box_loss_cpu.py finds between
                # the fixture and float64
                for key in ("loss_cls", "loss_box_reg"):
                    ref = float(fx[f"v_{name}_{key}"])
                    assert abs(float(o[key].detach()) - ref) <= 1.1e-5 * max(1, abs(ref)), (name, key)
                for g, ref in ((s2.grad, fx[f"v_{name}_grad_scores"]), (d2.grad, fx[f"v_{name}_grad_deltas"])):
                    assert (np.abs(g.cpu().numpy() - ref) <= 1.1e-5 * np.abs(ref) + 1e-6 / R).all(), name


def test_chaining_the_three_calls_over_the_fixtures_stages(fixture_on_device):
    """match -> losses -> next proposals, three times, as _forward_box does: the fixture's per-stage losses; the matcher's index goes on
    into mask_rcnn_loss_weighted unchanged."""
    from unmore_amd import box_loss as B
    from unmore_amd.mask_loss import mask_rcnn_loss_weighted
    fx, dev, N, targets = fixture_on_device
    single = _t(fx["single"], dev)
    sizes = [tuple(v) for v in fx["sizes"].tolist()]
    masks = [torch.ones((len(t["gt_boxes"]), sizes[k][0], sizes[k][1]), dtype=torch.bool, device=dev) for k, t in enumerate(targets)]
    targets = [dict(t, gt_masks=m) for t, m in zip(targets, masks)]
    props = [_t(fx[f"st0_im{k}_proposal_boxes"], dev) for k in range(N)]
    for s in range(3):
        matched = B.match_and_label(props, targets, STAGE_IOUS[s], 1)
        R = sum(len(m["proposal_boxes"]) for m in matched)
        assert R == len(fx[f"st{s}_scores"]), s
        scores, deltas = _t(fx[f"st{s}_scores"], dev).requires_grad_(True), _t(fx[f"st{s}_deltas"], dev).requires_grad_(True)
        out = B.fast_rcnn_losses(scores, deltas, matched, box2box_weights=STAGE_WEIGHTS[s], droploss=(float(fx["drop_thresh"]), single))
        for key in ("loss_cls", "loss_box_reg"):
            ref = float(fx[f"st{s}_{key}"])      # float32 torch: 1e-5 plus the 1e-6 between the fixture and float64 (tests/test_box_loss_cpu.py)
            assert abs(float(out[key].detach()) - ref) <= 1.1e-5 * max(1, abs(ref)), (s, key)
        boxes, keep, counts = B.next_stage_proposals(deltas, matched, STAGE_WEIGHTS[s], sizes)
        props = B.split_proposals(boxes, counts)
    fg = [m for m in matched]
    logits = torch.zeros((R, 1, 7, 7), device=dev, requires_grad=True)
    loss = mask_rcnn_loss_weighted(logits, fg, torch.cat([m["gt_scores"] for m in fg]))
    assert np.isfinite(float(loss)) and float(loss) > 0


def test_hand_worked_cases_on_the_device():
    """the hand-worked cases of tests/test_box_loss_cpu.py through the kernels themselves"""
    from unmore_amd import box_loss as B
    dev = _dev()

    def tgt(boxes, scores):
        return {"gt_boxes": torch.tensor(boxes, dtype=torch.float32, device=dev).reshape(-1, 4),
                "gt_classes": torch.zeros(len(boxes), dtype=torch.int64, device=dev), "gt_scores": torch.tensor(scores, dtype=torch.float32, device=dev)}

    def prop(boxes):
        return torch.tensor(boxes, dtype=torch.float32, device=dev).reshape(-1, 4)

    # IoU exactly 0.5 ([0,0,2,2] against [0,0,2,1]: 2 / (4 + 2 - 2)) is foreground at t = 0.5 and background at 0.6; touching boxes give 0;
    # a tie goes to the lower index (ground truths 1 and 2 of the second image are the same box)
    props = [prop([[0, 0, 2, 1], [2, 0, 4, 2], [0, 2, 2, 4], [5, 5, 6, 6]]), prop([[0, 0, 2, 2], [0, 0, 2, 1]])]
    targets = [tgt([[0, 0, 2, 2]], [0.7]), tgt([[10, 10, 12, 12], [0, 0, 2, 2], [0, 0, 2, 2]], [0.1, 0.2, 0.3])]
    st = {}
    m = B.match_and_label(props, targets, 0.5, stats=st)
    assert m[0]["matched_vals"].tolist() == [0.5, 0, 0, 0] and m[0]["gt_classes"].tolist() == [0, 1, 1, 1]
    assert m[0]["gt_scores"].tolist() == [np.float32(0.7)] * 4 and m[0]["gt_boxes"].tolist() == [[0, 0, 2, 2]] * 4      # gathered on background rows too
    assert m[1]["matched_idxs"].tolist() == [1, 1] and m[1]["matched_vals"].tolist() == [1.0, 0.5] and m[1]["gt_scores"].tolist() == [np.float32(0.2)] * 2
    assert st["num_fg"].tolist() == [1, 2] and st["num_bg"].tolist() == [3, 0] and st["bad"].tolist() == [0, 0]
    m = B.match_and_label(props, targets, 0.6, stats=st)
    assert st["num_fg"].tolist() == [0, 1] and m[0]["gt_classes"].tolist() == [1, 1, 1, 1] and m[1]["gt_classes"].tolist() == [0, 1]

    # decode: the clamp at log(1000 / 16), and a box that clips to zero width is dropped in training, kept at inference, order preserved
    box = prop([[10, 20, 30, 60]])
    big = B.apply_deltas(torch.tensor([[0, 0, 30.0, 0]], device=dev), box, W4)
    assert torch.equal(big, B.apply_deltas(torch.tensor([[0, 0, 300.0, 0]], device=dev), box, W4))
    width = float(big[0, 2] - big[0, 0])
    assert abs(width - 20 * 1000 / 16) <= 20 * 1000 / 16 * 4 * EPS32 and big[0, 1] == 20 and big[0, 3] == 60
    assert torch.equal(B.apply_deltas(torch.tensor([[5, -2.5, 0, 0]], device=dev), box, W4), prop([[20, 10, 40, 50]]))
    three = [prop([[10, 10, 20, 20]] * 3)]
    deltas = torch.tensor([[0, 0, 0, 0], [100, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.float32, device=dev)
    boxes, keep, counts = B.next_stage_proposals(deltas, three, W4, [(30, 40)])
    assert keep.tolist() == [True, False, True] and counts.tolist() == [2] and boxes[:2].tolist() == [[10, 10, 20, 20], [11, 10, 21, 20]]
    boxes, keep, counts = B.next_stage_proposals(deltas, three, W4, [(30, 40)], training=False)
    assert keep.all() and counts.tolist() == [3] and boxes.tolist() == [[10, 10, 20, 20], [40, 10, 40, 20], [11, 10, 21, 20]]

    # drop weights: the set is the first n rows of the matched boxes, n = the number of distinct rows -> {a, a}: the row on b finds nothing
    a, b = [0, 0, 4, 4], [10, 10, 14, 14]
    item = {"proposal_boxes": prop([a, a, b]), "gt_boxes": prop([a, a, b])}
    assert B.droploss_weights(torch.zeros(3, 4, device=dev), [item], W4, 0.01).tolist() == [1, 1, 0]

    # the single-object indicator by position r // (R // N); every row's IoU with its set is 0
    def far(n):
        return {"proposal_boxes": prop([a] * n), "gt_boxes": prop([b] * n)}
    for rows, single, want in (((3, 2), [0, 1], [0, 0, 1, 1, 0]), ((3, 2), [1, 0], [1, 1, 0, 0, 0]), ((2, 2, 1), [1, 1, 1], [1, 1, 1, 0, 0]),
                               ((1, 1, 0), [1, 1, 1], [0, 0]), ((3, 2), None, [0, 0, 0, 0, 0])):
        R = sum(rows)
        got = B.droploss_weights(torch.zeros(R, 4, device=dev), [far(n) for n in rows], W4, 0.01,
                                 None if single is None else torch.tensor(single, device=dev))
        assert got.tolist() == want, (rows, single)


def test_more_than_256_chunks_reach_the_strided_part_of_the_finishing_sum():
    """257 images of one proposal and one matched ground truth each: every image starts a chunk of its own, so the finishing launch adds
    257 partials and its thread 0 adds partial 0 and partial 256.  Weights, scores and a few background rows make every partial differ."""
    from unmore_amd import box_loss as B
    dev, N = _dev(), 257
    rng = np.random.RandomState(257)
    xy, wh = rng.uniform(0, 80, (N, 2)), rng.uniform(8, 40, (N, 2))
    gb = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    pb = (gb + rng.uniform(-0.2, 0.2, (N, 4)) * np.tile(wh, 2)).astype(np.float32)
    gc = (rng.uniform(size=N) < 0.25).astype(np.int64)                 # 1 == num_classes: background
    gs, w = rng.uniform(0.2, 1.0, N).astype(np.float32), rng.uniform(0.0, 2.0, N).astype(np.float32)
    scores = (rng.standard_normal((N, 2)) * 3).astype(np.float32)
    deltas = (rng.standard_normal((N, 4)) * np.array(W4) * 0.05).astype(np.float32)
    lc, lb, _, _, counters = losses_reference(scores, deltas, pb, gb, gc, gs, w, W4)
    items = [{"proposal_boxes": _t(pb[k:k + 1], dev), "gt_boxes": _t(gb[k:k + 1], dev), "gt_classes": _t(gc[k:k + 1], dev),
              "gt_scores": _t(gs[k:k + 1], dev)} for k in range(N)]
    runs = []
    for _ in range(2):
        s, d = _t(scores, dev).requires_grad_(True), _t(deltas, dev).requires_grad_(True)
        st = {}
        out = B.fast_rcnn_losses(s, d, items, box2box_weights=W4, weights=_t(w, dev), stats=st)
        (out["loss_cls"] + out["loss_box_reg"]).backward()
        runs.append((out["loss_cls"].detach(), out["loss_box_reg"].detach(), st["counters"], s.grad, d.grad))
    got_c, got_b = float(runs[0][0]), float(runs[0][1])
    print(f"loss_cls {got_c!r} (float64 {lc!r}), loss_box_reg {got_b!r} (float64 {lb!r})")
    assert abs(got_c - lc) <= 1e-5 * max(1, abs(lc)) and abs(got_b - lb) <= 1e-5 * max(1, abs(lb))
    assert runs[0][2].tolist() == counters and counters[0] == N and 0 < counters[1] < N and counters[6] == 0
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(runs[0][3].view(torch.int32), runs[1][3].view(torch.int32)) and torch.equal(runs[0][4].view(torch.int32), runs[1][4].view(torch.int32))
