"""unmore_amd.roi_sample on the MI355X against the restatement of tests/roi_sample_common.py and the fixture recorded from the reference.
Every output is an integer decision, a copy of an input or a float32 value that NumPy reproduces bit for bit, so everything must be
EQUAL: there is no tolerance.  The output buffers of the padded form lie between sentinel guards that must stay intact."""
import numpy as np
import pytest
import torch

import roi_sample_common as C

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64                   # sentinel bytes times 16 on either side of every guarded allocation
SENTINEL = 0xa5


def _dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _to_device(props, tgts, scores=True):
    dev = _dev()
    p = [{"proposal_boxes": torch.from_numpy(b).to(dev), "objectness_logits": torch.from_numpy(l).to(dev)} for b, l in props]
    t = [{k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in g.items() if scores or k != "gt_scores"} for g in tgts]
    return p, t


def _keys_t(keys):
    return None if keys is None else [torch.from_numpy(np.asarray(k, np.int64).astype(np.int32)).to(_dev()) for k in keys]


def _call(props, tgts, case, keys=None, scores=True, **kw):
    from unmore_amd import roi_sample
    p, t = _to_device(props, tgts, scores)
    st = {}
    args = {"iou_threshold": case["threshold"], "num_classes": case["num_classes"], "batch_size_per_image": case["B"],
            "positive_fraction": case["fraction"], "seed": case["seed"]}
    args.update(kw)
    out = roi_sample.label_and_sample_proposals(p, t, keys=_keys_t(keys), stats=st, **args)
    return out, st


def _assert_rows(got, r, n, scores=True):
    """the rows of one image (a dict of arrays, cut to the count) EQUAL the restatement's"""
    for name in ("proposal_boxes", "objectness_logits", "gt_boxes") + (("gt_scores",) if scores else ()):
        assert np.array_equal(_bits(got[name]), _bits(r[name])), (n, name)
    for name in ("gt_classes", "matched_idxs", "sampled_idxs"):
        assert np.array_equal(got[name], r[name]), (n, name)
    assert ("gt_scores" in got) == scores


def _assert_list(out, st, ref, scores=True):
    from unmore_amd import roi_sample
    assert isinstance(out, roi_sample.Samples) and len(out) == len(ref)
    assert out.counts == [list(r["counts"]) for r in ref]
    for n, (item, r) in enumerate(zip(out, ref)):
        assert item["gt_classes"].dtype == torch.int64 and item["matched_idxs"].dtype == torch.int64 and item["sampled_idxs"].dtype == torch.int32
        assert item["mask_index"] is item["matched_idxs"] and item["proposal_boxes"].is_cuda and item["proposal_boxes"].is_contiguous()
        _assert_rows({k: v.cpu().numpy() for k, v in item.items() if isinstance(v, torch.Tensor)}, r, n, scores)
    _assert_stats(st, ref)


def _assert_stats(st, ref):
    assert st["counters"].dtype == torch.int32 and st["counters"].is_cuda
    assert np.array_equal(st["counters"].cpu().numpy(), np.stack([r["counters"] for r in ref]))
    for n, r in enumerate(ref):                                                         # the match launch, every candidate: bl_iou's bits
        assert np.array_equal(_bits(st["matched_vals"][n].cpu().numpy()), _bits(r["all_vals"])), n
        assert np.array_equal(st["matched_idxs"][n].cpu().numpy(), r["all_idx"]), n
    N = len(ref)
    assert st["scalars"]() == {"roi_head/num_fg_samples": sum(r["counts"][0] for r in ref) / N,
                               "roi_head/num_bg_samples": sum(r["counts"][1] for r in ref) / N, "bad": int(sum(r["counters"][4] for r in ref))}


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("order", ["key", "index"])
@pytest.mark.parametrize("keys", [None, "base"])
@pytest.mark.parametrize("append", [True, False])
def test_base_batch_equals_the_restatement(order, keys, append):
    props, tgts = C.base_batch()
    kw = {"order": order, "append_gt": append}
    if keys:
        kw["keys"] = "base"
    ref = C.reference("base", **kw)
    out, st = _call(props, tgts, C.BASE, keys=C.base_keys(append_gt=append) if keys else None, order=order, proposal_append_gt=append)
    _assert_list(out, st, ref)


def test_flat_keys_and_no_scores_equal_the_restatement():
    from unmore_amd import roi_sample
    props, tgts = C.base_batch()
    ref = C.reference("base", keys="base")
    p, t = _to_device(props, tgts, scores=False)
    flat = torch.cat(_keys_t(C.base_keys()))
    c, st = C.BASE, {}
    out = roi_sample.label_and_sample_proposals([(d["proposal_boxes"], d["objectness_logits"]) for d in p], t, iou_threshold=c["threshold"],
                                                batch_size_per_image=c["B"], positive_fraction=c["fraction"], keys=flat, stats=st)
    _assert_list(out, st, ref, scores=False)


def test_big_batch_equals_the_restatement():
    props, tgts = C.big_batch()
    out, st = _call(props, tgts, C.BIG)
    _assert_list(out, st, C.reference("big"))


def test_fixture_rows_equal_the_reference_row_for_row():
    from unmore_amd import roi_sample
    fx = C.load_fixture()
    props, tgts, keys = C.fixture_batch(fx)
    case = {"threshold": float(fx["iou_threshold"]), "num_classes": int(fx["num_classes"]), "B": int(fx["batch_size_per_image"]),
            "fraction": float(fx["positive_fraction"]), "seed": 0}
    out, st = _call(props, tgts, case, keys=keys)
    for k, item in enumerate(out):
        assert np.array_equal(item["sampled_idxs"].cpu().numpy(), fx[f"im{k}_sampled_idxs"]), k
        for name in ("proposal_boxes", "objectness_logits", "gt_boxes", "gt_scores"):
            assert np.array_equal(_bits(item[name].cpu().numpy()), _bits(fx[f"im{k}_out_{name}"])), (k, name)
        assert np.array_equal(item["gt_classes"].cpu().numpy(), fx[f"im{k}_out_gt_classes"]), k
    s = st["scalars"]()
    assert [s["roi_head/num_fg_samples"], s["roi_head/num_bg_samples"]] == fx["scalars"].tolist() and s["bad"] == 0
    # the append alone, on the device
    p, t = _to_device(props, tgts)
    for (boxes, logits), (b, l), g in zip(roi_sample.add_ground_truth_to_proposals(t, p), props, tgts):
        assert np.array_equal(_bits(boxes.cpu().numpy()), _bits(np.concatenate([b, g["gt_boxes"]])))
        assert np.array_equal(_bits(logits.cpu().numpy()), _bits(np.concatenate([l, np.full(len(g["gt_boxes"]), C.GT_LOGIT, F32)])))


# ---------------------------------------------------------------------------------------------------------------- the padded form
class _Guarded:
    """an allocator whose tensors lie between GUARD * 16 sentinel bytes in one allocation each, pre-filled with the sentinel"""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        pad = GUARD * 16
        buf = torch.full((pad + (n + 15) // 16 * 16 + pad,), SENTINEL, dtype=torch.uint8, device=_dev())
        self.bufs.append((buf, pad, n))
        return buf[pad:pad + n].view(dtype).view(shape)

    def intact(self):
        return all(bool((b[:pad] == SENTINEL).all()) and bool((b[pad + n:] == SENTINEL).all()) for b, pad, n in self.bufs)


@pytest.mark.parametrize("order", ["key", "index"])
def test_padded_form_equals_the_restatement_inside_its_guards(order):
    props, tgts = C.base_batch()
    ref = C.reference("base", order=order)
    alloc = _Guarded()
    out, st = _call(props, tgts, C.BASE, order=order, padded=True, _alloc=alloc)
    assert isinstance(out, dict) and out["counts"].dtype == torch.int32 and out["counts"].is_cuda
    assert len(alloc.bufs) == 10 and alloc.intact(), "a launch wrote outside a buffer"
    B = C.BASE["B"]
    counts = out["counts"].cpu().numpy()
    assert counts.tolist() == [list(r["counts"]) for r in ref]
    host = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
    for n, r in enumerate(ref):
        S = sum(r["counts"])
        assert host["proposal_boxes"].shape == (len(ref), B, 4) and host["gt_classes"].shape == (len(ref), B)
        _assert_rows({k: v[n, :S] for k, v in host.items() if k != "counts"}, r, n)
        for name in ("proposal_boxes", "objectness_logits", "gt_boxes", "gt_scores", "matched_idxs", "sampled_idxs"):
            assert not host[name][n, S:].view(np.uint8).any(), (n, name)                # rows past the count: zero bytes
        assert (host["gt_classes"][n, S:] == -1).all(), n
    _assert_stats(st, ref)
    from unmore_amd import roi_sample
    fg = roi_sample.foreground(out).cpu().numpy()
    assert np.array_equal(fg, (host["gt_classes"] != C.BASE["num_classes"]) & (host["gt_classes"] != -1))


# ---------------------------------------------------------------------------------------------------------------- streams, repeatability
def test_a_second_run_and_a_side_stream_give_identical_bytes():
    props, tgts = C.base_batch()
    ref = C.reference("base")
    a, _ = _call(props, tgts, C.BASE)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b, st = _call(props, tgts, C.BASE)
    side.synchronize()
    _assert_list(b, st, ref)
    for name, v in a.padded.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v.view(torch.uint8), b.padded[name].view(torch.uint8)), name


def test_foreground_is_the_rows_that_are_not_background():
    from unmore_amd import roi_sample
    props, tgts = C.base_batch()
    out, _ = _call(props, tgts, C.BASE)
    fg = roi_sample.foreground(out)
    assert len(fg) == len(out)
    for item, f in zip(out, fg):
        keep = (item["gt_classes"] != C.BASE["num_classes"]).cpu().numpy()
        n = int(keep.sum())
        assert keep[:n].all() and not keep[n:].any()                                    # the foreground rows are a prefix
        for name in ("proposal_boxes", "objectness_logits", "gt_classes", "gt_boxes", "gt_scores", "matched_idxs", "mask_index", "sampled_idxs"):
            assert torch.equal(f[name], item[name][torch.from_numpy(keep).to(_dev())]), name
            assert f[name].data_ptr() == item[name].data_ptr() or n == 0                # a view, not a copy


# ---------------------------------------------------------------------------------------------------------------- downstream
def test_the_dicts_run_through_the_losses_and_the_pooler():
    from unmore_amd import box_loss, mask_loss, roi_pool, roi_sample
    props, tgts = C.base_batch()
    props, tgts = [props[0], props[5]], [tgts[0], tgts[5]]
    dev = _dev()
    rng = np.random.RandomState(2)
    h, w = C.BASE["frame"]
    p, t = _to_device(props, tgts)
    for g in t:
        g["gt_masks"] = torch.from_numpy(rng.rand(len(g["gt_boxes"]), h, w) > 0.5).to(dev)
    c = C.BASE
    out = roi_sample.label_and_sample_proposals(p, t, iou_threshold=c["threshold"], batch_size_per_image=c["B"],
                                                positive_fraction=c["fraction"], seed=c["seed"])
    assert all(item["gt_masks"] is g["gt_masks"] for item, g in zip(out, t))
    R = sum(len(item["gt_classes"]) for item in out)
    scores = torch.from_numpy(rng.standard_normal((R, 2)).astype(F32)).to(dev).requires_grad_(True)
    deltas = torch.from_numpy((rng.standard_normal((R, 4)) * 0.1).astype(F32)).to(dev).requires_grad_(True)
    losses = box_loss.fast_rcnn_losses(scores, deltas, out, box2box_weights=(10.0, 10.0, 5.0, 5.0), droploss=(0.01, None))
    assert all(bool(torch.isfinite(v.detach())) for v in losses.values()) and float(losses["loss_box_reg"].detach()) > 0
    feats = [torch.from_numpy(rng.standard_normal((2, 8, 16, 16)).astype(F32)).to(dev)]
    pooled = roi_pool.ROIPooler(7, [0.25], sampling_ratio=2)(feats, [item["proposal_boxes"] for item in out])
    assert tuple(pooled.shape) == (R, 8, 7, 7) and bool(torch.isfinite(pooled).all())
    fg = roi_sample.foreground(out)
    Rf = sum(len(item["gt_classes"]) for item in fg)
    assert Rf == sum(n for n, _ in out.counts) > 0
    logits = torch.from_numpy(rng.standard_normal((Rf, 1, 14, 14)).astype(F32)).to(dev).requires_grad_(True)
    loss = mask_loss.mask_rcnn_loss_weighted(logits, fg, torch.cat([item["gt_scores"] for item in fg]))
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    stage1 = box_loss.match_and_label(out, t, 0.6)
    assert [len(s["gt_classes"]) for s in stage1] == [len(item["gt_classes"]) for item in out]


# ---------------------------------------------------------------------------------------------------------------- the hash draw
def test_the_hash_draw_on_the_device_is_the_restatement_and_uniform_enough():
    """the seeds and bounds of tests/test_roi_sample_cpu.py::test_the_hash_draw_is_uniform_enough: expectation 12.8 of 64, bounds [3, 25]"""
    from unmore_amd import roi_sample
    props, tgts = C.hash_draw_batch()
    p, t = _to_device(props, tgts)
    times = np.zeros(100, np.int64)
    padded = [roi_sample.label_and_sample_proposals(p, t, batch_size_per_image=32, positive_fraction=0.25, proposal_append_gt=False,
                                                    seed=seed, padded=True) for seed in C.HASH_SEEDS]
    rows = torch.stack([o["sampled_idxs"][0] for o in padded]).cpu().numpy()
    counts = torch.stack([o["counts"][0] for o in padded]).cpu().numpy()
    for seed, row, cnt in zip(C.HASH_SEEDS, rows, counts):
        r, = C.label_and_sample_np(props, tgts, 0.5, 1, 32, 0.25, append_gt=False, seed=seed)
        assert cnt.tolist() == [8, 24] and np.array_equal(row, r["sampled_idxs"]), seed
        times[row[:8]] += 1
    assert times[40:].sum() == 0 and times[:40].min() >= 3 and times[:40].max() <= 25, times[:40]
