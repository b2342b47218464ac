"""unmore_amd.rpn_loss on the MI355X against the restatement of tests/rpn_loss_common.py.  Matching, labelling and sampling are integer
decisions on float32 values that NumPy reproduces bit for bit, so everything up to the samples must be EQUAL.  The losses are compared
with the float64 restatement on the device's own samples at the project's tolerances (tests/test_mask_loss_gpu.py): losses 1e-5 *
max(1, |loss64|); float32 gradients 1e-5 relative + 1e-6 / (number of gradient elements); bfloat16 gradients within one bfloat16 ulp of
float64.  The tests print the worst errors as shares of these bounds."""
import numpy as np
import pytest
import torch

import rpn_common as RC
import rpn_loss_common as C

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _cells_t(cells):
    return [torch.from_numpy(np.asarray(c, F32)) for c in cells]


def _label(cells, strides, maps, gts, sizes, **kw):
    """one call with the debug and dense returns: (samples, everything as NumPy in a dict)"""
    from unmore_amd import rpn_loss
    dev = _dev()
    dbg, st = {}, {}
    if kw.get("keys") is not None:
        kw["keys"] = torch.from_numpy(np.ascontiguousarray(kw["keys"], dtype=np.int32)).to(dev)
    s = rpn_loss.label_and_sample_anchors(_cells_t(cells), list(strides), list(maps), [torch.from_numpy(np.asarray(g, F32).reshape(-1, 4)).to(dev)
                                                                                      for g in gts], list(sizes), dense=True, stats=st,
                                          _debug=dbg, **kw)
    assert s.index.dtype == torch.int32 and s.gt.dtype == torch.int32 and s.counts.dtype == torch.int32 and s.index.is_cuda
    assert st["counters"].dtype == torch.int32 and st["counters"].is_cuda and s.labels.dtype == torch.int8
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in dbg.items()}
    got.update(index=s.index.cpu().numpy(), gt=s.gt.cpu().numpy(), counts=s.counts.cpu().numpy(), dense=s.labels.cpu().numpy(),
               dense_idx=s.matched_idxs.cpu().numpy(), counters=st["counters"].cpu().numpy(), scalars=st["scalars"]())
    return s, got


def _assert_equal(got, ref):
    """everything the device wrote EQUALS the restatement"""
    first = got["gt_first"]
    for n, r in enumerate(ref):
        assert np.array_equal(_bits(got["matched_vals"][n]), _bits(r["vals"])), n
        assert np.array_equal(got["matched_idxs"][n], r["idx"]), n
        assert np.array_equal(_bits(got["row_max"][first[n]:first[n + 1]]), _bits(r["row_max"])), n
        assert np.array_equal(got["labels"][n], r["labels"]), n
        p, q = len(r["pos"]), len(r["neg"])
        assert got["counts"][n].tolist() == [p, q], n
        assert np.array_equal(got["index"][n, :p], r["pos"]) and np.array_equal(got["index"][n, p:p + q], r["neg"]), n
        assert np.array_equal(got["gt"][n, :p + q], r["gt"]), n
        assert got["counters"][n].tolist() == r["counters"].tolist(), n
        assert np.array_equal(got["dense"][n], r["dense"]) and np.array_equal(got["dense_idx"][n], r["idx"]), n
    N = len(ref)
    assert got["scalars"] == {"rpn/num_pos_anchors": sum(len(r["pos"]) for r in ref) / N, "rpn/num_neg_anchors": sum(len(r["neg"]) for r in ref) / N,
                              "bad": sum(r["bad"] for r in ref)}


def _base():
    c = C.BASE
    return C.base_cells(), c["strides"], c["maps"], C.base_gt(), c["image_sizes"]


# ---------------------------------------------------------------------------------------------------------------- exactness
def test_base_case_equals_the_restatement():
    c = C.BASE
    _, got = _label(*_base(), batch_size_per_image=c["B"], positive_fraction=c["fraction"], seed=c["seed"])
    _assert_equal(got, C.base_reference())


def test_base_case_inside_the_frames_equals_the_restatement():
    c = C.BASE
    _, got = _label(*_base(), batch_size_per_image=c["B"], positive_fraction=c["fraction"], seed=c["seed"], anchor_boundary_thresh=0)
    _assert_equal(got, C.base_reference(boundary=0))


@pytest.mark.parametrize("kind", ["drawn", "few_values", "all_equal"])
def test_base_case_with_given_keys_equals_the_restatement(kind):
    c = C.BASE
    R = sum(h * w for h, w in c["maps"]) * c["A"]
    rng = np.random.RandomState(11)
    keys = {"drawn": rng.randint(0, 1 << 31, (c["N"], R)), "few_values": rng.randint(0, 7, (c["N"], R)),
            "all_equal": np.full((c["N"], R), 12345)}[kind]                                 # all equal: the order is by index alone
    cells, strides, maps, gts, sizes = _base()
    _, got = _label(cells, strides, maps, gts, sizes, batch_size_per_image=c["B"], positive_fraction=c["fraction"], keys=keys)
    ref = C.label_and_sample_np(cells, strides, maps, gts, sizes, c["B"], c["fraction"], keys=keys)
    _assert_equal(got, ref)
    if kind == "all_equal":
        for n, r in enumerate(ref):
            assert np.array_equal(r["pos"], np.nonzero(r["labels"] == 1)[0][:len(r["pos"])])


# ---------------------------------------------------------------------------------------------------------------- losses
def _predictions(dtype=torch.float32):
    logits, deltas = C.base_predictions()
    dev = _dev()
    lg = [torch.from_numpy(x).to(dev).to(dtype).requires_grad_(True) for x in logits]
    dl = [torch.from_numpy(x).to(dev).to(dtype).requires_grad_(True) for x in deltas]
    return lg, dl


def _samples_np(got):
    out = []
    for n in range(len(got["counts"])):
        p, q = got["counts"][n]
        out.append((got["index"][n, :p], got["index"][n, p:p + q], got["gt"][n, :p]))
    return out


_base_samples = {}


def _base_call():
    """label_and_sample_anchors on the base case, once: (samples on the device, as NumPy)"""
    if not _base_samples:
        c = C.BASE
        _base_samples["s"], _base_samples["got"] = _label(*_base(), batch_size_per_image=c["B"], positive_fraction=c["fraction"], seed=c["seed"])
    return _base_samples["s"], _base_samples["got"]


def _run_losses(dtype, weights, beta, loss_weight):
    """(loss_cls, loss_loc, gradient maps) of the device and of the float64 restatement on the device's samples and the values it read"""
    from unmore_amd import rpn_loss
    c = C.BASE
    s, got = _base_call()
    lg, dl = _predictions(dtype)
    out = rpn_loss.rpn_losses(lg, dl, s, _cells_t(C.base_cells()), list(c["strides"]), [torch.from_numpy(g).to(_dev()) for g in C.base_gt()],
                              box2box_weights=weights, smooth_l1_beta=beta, batch_size_per_image=c["B"], loss_weight=loss_weight)
    assert set(out) == {"loss_rpn_cls", "loss_rpn_loc"} and all(v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda for v in out.values())
    (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()
    assert all(t.grad.dtype == dtype and t.grad.shape == t.shape for t in lg + dl)
    lw = (loss_weight.get("loss_rpn_cls", 1.0), loss_weight.get("loss_rpn_loc", 1.0)) if isinstance(loss_weight, dict) else (loss_weight,) * 2
    read = [t.detach().float().cpu().numpy() for t in lg + dl]
    nl = len(lg)
    want = C.losses_np(read[:nl], read[nl:], _samples_np(got), C.base_cells(), c["strides"], C.base_gt(), c["B"], weights, beta, lw)
    grads = [t.grad.float().cpu().numpy().astype(np.float64) for t in lg + dl]
    return (out["loss_rpn_cls"].item(), out["loss_rpn_loc"].item(), grads), (want[0], want[1], want[2] + want[3]), want[4]


@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_losses_and_gradients_float32(weights, beta):
    lw = {"loss_rpn_cls": 2.0, "loss_rpn_loc": 0.25} if beta == 0.5 else 1.0                # a loss_weight dict in half of the cases
    got, want, _ = _run_losses(torch.float32, weights, beta, lw)
    shares = [abs(got[k] - want[k]) / (1e-5 * max(1.0, abs(want[k]))) for k in (0, 1)]
    n = sum(g.size for g in got[2])
    worst = 0.0
    for g, w in zip(got[2], want[2]):
        assert np.array_equal(g != 0, w != 0)                                               # exactly zero outside the samples
        worst = max(worst, float((np.abs(g - w) / (1e-5 * np.abs(w) + 1e-6 / n)).max()))
    print(f"rpn_losses float32 weights {weights} beta {beta}: loss errors {shares[0]:.3f} / {shares[1]:.3f} of their bounds, "
          f"worst gradient error {worst:.3f} of its bound ({n} gradient elements)")
    assert max(shares) <= 1.0 and worst <= 1.0


def test_losses_and_gradients_bfloat16():
    got, want, _ = _run_losses(torch.bfloat16, (10.0, 10.0, 5.0, 5.0), 0.5, 1.0)
    shares = [abs(got[k] - want[k]) / (1e-5 * max(1.0, abs(want[k]))) for k in (0, 1)]    # the losses are float32 of the widened inputs
    worst = 0.0
    for g, w in zip(got[2], want[2]):
        assert np.array_equal(g != 0, w != 0)
        nz = w != 0
        ulp = 2.0 ** (np.floor(np.log2(np.abs(w[nz]))) - 7)                                  # bfloat16: 8 bits of significand
        worst = max(worst, float((np.abs(g[nz] - w[nz]) / ulp).max()) if nz.any() else 0.0)
    print(f"rpn_losses bfloat16: loss errors {shares[0]:.3f} / {shares[1]:.3f} of their bounds, worst gradient error {worst:.3f} bfloat16 ulp")
    assert max(shares) <= 1.0 and worst <= 1.0


def test_backward_scales_the_saved_maps():
    from unmore_amd import rpn_loss
    c = C.BASE
    s, _ = _base_call()
    gts = [torch.from_numpy(g).to(_dev()) for g in C.base_gt()]
    grads = []
    for scale in (1.0, 0.37):
        lg, dl = _predictions()
        out = rpn_loss.rpn_losses(lg, dl, s, _cells_t(C.base_cells()), list(c["strides"]), gts, batch_size_per_image=c["B"])
        (scale * out["loss_rpn_cls"] + scale * out["loss_rpn_loc"]).backward()
        grads.append([t.grad for t in lg + dl])
    for a, b in zip(*grads):
        assert torch.allclose(b, 0.37 * a, rtol=1e-6, atol=0)
    # each loss reaches its own maps only
    lg, dl = _predictions()
    out = rpn_loss.rpn_losses(lg, dl, s, _cells_t(C.base_cells()), list(c["strides"]), gts, batch_size_per_image=c["B"])
    out["loss_rpn_loc"].backward()
    assert all(not t.grad.any() for t in lg) and any(t.grad.any() for t in dl)


def test_the_localisation_sum_agrees_with_the_reference_fixture():
    fx = C.load_fixture()
    c = C.BASE
    for name, weights, beta in (("w1_b0", (1.0, 1.0, 1.0, 1.0), 0.0), ("w10_b05", (10.0, 10.0, 5.0, 5.0), 0.5)):
        got, _, _ = _run_losses(torch.float32, weights, beta, 1.0)
        want = float(fx[f"sum_{name}"])
        assert abs(got[1] * c["B"] * c["N"] - want) <= 1e-5 * abs(want), name


# ---------------------------------------------------------------------------------------------------------------- edges
def _check_case(cells, strides, maps, gts, sizes, B, fraction=0.5, **kw):
    s, got = _label(cells, strides, maps, gts, sizes, batch_size_per_image=B, positive_fraction=fraction, **kw)
    ref = C.label_and_sample_np(cells, strides, maps, gts, sizes, B, fraction, seed=kw.get("seed", 0), boundary=kw.get("anchor_boundary_thresh", -1))
    _assert_equal(got, ref)
    return s, got, ref


def test_no_ground_truths_in_any_image():
    c = C.BASE
    _, got, _ = _check_case(C.base_cells(), c["strides"], c["maps"], [np.zeros((0, 4), F32)] * 2, c["image_sizes"][:2], 64, seed=4)
    assert got["counts"].tolist() == [[0, 64], [0, 64]] and not got["matched_idxs"].any()


def test_one_tiny_level_where_both_classes_fall_short():
    cells = [RC.cell_anchors_np((32,), (1.0,))]
    gts = [np.array([[0, 0, 30, 30]], F32)]
    _, got, ref = _check_case(cells, (16,), ((2, 2),), gts, ((32, 32),), 16, seed=9)
    assert got["counts"].sum() < 16 and got["counts"][0, 0] >= 1 and got["counts"][0, 1] >= 1
    assert got["counts"].sum() == int((ref[0]["labels"] >= 0).sum())


def test_three_hundred_ground_truths_cross_the_lds_tile():
    c = C.BASE
    rng = np.random.RandomState(21)
    xy = rng.uniform(0, 1, (300, 2)) * np.array([200.0, 140.0])
    wh = rng.uniform(6, 20, (300, 2))
    gts = [np.concatenate([xy, xy + wh], axis=1).astype(F32)]
    _, got, ref = _check_case(C.base_cells(), c["strides"], c["maps"], gts, ((160, 224),), 256, seed=2)
    assert ref[0]["idx"].max() >= 256 and got["counts"][0, 0] == 128                        # matches beyond the first tile


def test_a_single_large_level():
    cells = [RC.cell_anchors_np((32,), (0.5, 1.0, 2.0))]
    rng = np.random.RandomState(8)
    xy = rng.uniform(0, 1, (5, 2)) * np.array([500.0, 500.0])
    gts = [np.concatenate([xy, xy + rng.uniform(20, 90, (5, 2))], axis=1).astype(F32)]
    _, got, ref = _check_case(cells, (4,), ((150, 152),), gts, ((600, 608),), 256, seed=12)
    assert got["matched_vals"].shape == (1, 68400) and got["index"][0, :got["counts"][0].sum()].max() > 1 << 16


@pytest.mark.parametrize("hw", [(128, 128), (113, 145)])
def test_at_the_threshold_between_one_and_two_select_steps(hw):
    """R = 16384 is sampled by one select, R = 16385 by partial selects (the second part holds one anchor) and a select over their
    survivors; keys of a few values put ties inside and across the parts"""
    from unmore_amd import rpn_loss
    assert hw[0] * hw[1] - rpn_loss.SELECT_SHARE == (0 if hw == (128, 128) else 1)
    cells = [RC.cell_anchors_np((24,), (1.0,))]
    rng = np.random.RandomState(hw[0])
    xy = rng.uniform(0, 1, (4, 2)) * np.array([400.0, 400.0])
    gts = [np.concatenate([xy, xy + rng.uniform(16, 60, (4, 2))], axis=1).astype(F32)]
    keys = rng.randint(0, 5, (1, hw[0] * hw[1]))
    keys[0, -1] = 9                                                                         # the lone anchor of the second part is taken
    sizes = ((hw[0] * 4, hw[1] * 4),)
    _, got = _label(cells, (4,), (hw,), gts, sizes, batch_size_per_image=64, positive_fraction=0.25, keys=keys)
    ref = C.label_and_sample_np(cells, (4,), (hw,), gts, sizes, 64, 0.25, keys=keys)
    _assert_equal(got, ref)
    assert ref[0]["labels"][-1] == 0 and ref[0]["neg"][-1] == hw[0] * hw[1] - 1 and got["counts"][0].sum() == 64


def test_a_ground_truth_outside_every_anchor():
    c = C.BASE
    gts = [np.array([[20, 20, 90, 80], [5000, 5000, 5040, 5040]], F32)]
    _, got, ref = _check_case(C.base_cells(), c["strides"], c["maps"], gts, ((160, 224),), 64, seed=1)
    assert ref[0]["row_max"][1] == 0 and (got["labels"] == 1).all() and got["counters"][0].tolist() == [8961, 0, 32, 0, 0]


def test_a_nan_ground_truth_is_counted_and_changes_nothing_else():
    c = C.BASE
    gts = C.base_gt()
    with_nan = [np.concatenate([g[:1] * np.array([np.nan, 1, 1, 1], F32), g]).astype(F32) if n == 0 else g for n, g in enumerate(gts)]
    _, got, ref = _check_case(C.base_cells(), c["strides"], c["maps"], with_nan, c["image_sizes"], c["B"], seed=c["seed"])
    base = C.base_reference()
    assert got["counters"][:, 4].tolist() == [1, 0, 0, 0]
    for n in range(c["N"]):
        assert np.array_equal(got["labels"][n], base[n]["labels"]) and np.array_equal(_bits(got["matched_vals"][n]), _bits(base[n]["vals"]))
        assert np.array_equal(got["matched_idxs"][n], base[n]["idx"] + (1 if n == 0 else 0))
        p, q = got["counts"][n]
        assert np.array_equal(got["index"][n, :p], base[n]["pos"]) and np.array_equal(got["index"][n, p:p + q], base[n]["neg"])


# ---------------------------------------------------------------------------------------------------------------- determinism, other forms
def test_two_calls_give_the_same_bytes_and_two_seeds_differ():
    from unmore_amd import rpn_loss
    c = C.BASE
    runs = [_label(*_base(), batch_size_per_image=c["B"], positive_fraction=c["fraction"], seed=sd) for sd in (c["seed"], c["seed"], c["seed"] + 1)]
    (s0, a), (s1, b), (_, other) = runs
    for k in ("matched_vals", "matched_idxs", "row_max", "labels", "counts", "dense", "counters"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["counts"], other["counts"])
    for n in range(c["N"]):
        p, q = a["counts"][n]
        assert np.array_equal(a["index"][n, :p + q], b["index"][n, :p + q]) and np.array_equal(a["gt"][n, :p + q], b["gt"][n, :p + q])
        assert not np.array_equal(a["index"][n, :p + q], other["index"][n, :p + q]), n
    gts = [torch.from_numpy(g).to(_dev()) for g in C.base_gt()]
    outs = []
    for s in (s0, s1):
        lg, dl = _predictions()
        out = rpn_loss.rpn_losses(lg, dl, s, _cells_t(C.base_cells()), list(c["strides"]), gts, batch_size_per_image=c["B"], smooth_l1_beta=0.5)
        (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()
        outs.append([out["loss_rpn_cls"].detach(), out["loss_rpn_loc"].detach()] + [t.grad for t in lg + dl])
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def test_dense_labels_agree_with_the_compact_form():
    _, got = _base_call()
    for n in range(len(got["counts"])):
        p, q = got["counts"][n]
        want = np.full(got["dense"].shape[1], -1, np.int8)
        want[got["index"][n, :p]], want[got["index"][n, p:p + q]] = 1, 0
        assert np.array_equal(got["dense"][n], want)
        assert np.array_equal(got["gt"][n, :p + q], got["dense_idx"][n][got["index"][n, :p + q]])
        assert (np.diff(got["index"][n, :p]) > 0).all() and (np.diff(got["index"][n, p:p + q]) > 0).all()


def test_a_hand_worked_case():
    """one level of 1 x 2 positions, stride 16, one cell anchor (-8, -8, 8, 8): anchors (-8, -8, 8, 8) and (8, -8, 24, 8).  The ground
    truth IS anchor 0 (IoU 1: label 1) and only touches anchor 1 (IoU 0: label 0).  B = 2, so 1 / (B N) = 1 / 2.  Logits 0 and 0: each
    term is log 2, loss_rpn_cls = log 2, gradients (0.5 - 1) / 2 and 0.5 / 2.  The target deltas of anchor 0 are 0; its predicted deltas
    (1, -2, 0, 0.5) give L1 = 3.5, loss_rpn_loc = 1.75, gradients sign / 2 with 0 at 0; anchor 1's deltas get none."""
    from unmore_amd import rpn_loss
    dev = _dev()
    cells = [np.array([[-8, -8, 8, 8]], F32)]
    gts = [np.array([[-8, -8, 8, 8]], F32)]
    s, got = _label(cells, (16,), ((1, 2),), gts, ((16, 32),), batch_size_per_image=2)
    assert got["labels"].tolist() == [[1, 0]] and got["matched_vals"].tolist() == [[1.0, 0.0]] and got["row_max"].tolist() == [1.0]
    assert got["index"].tolist() == [[0, 1]] and got["gt"].tolist() == [[0, 0]] and got["counts"].tolist() == [[1, 1]]
    assert got["counters"].tolist() == [[1, 1, 1, 1, 0]] and got["dense"].tolist() == [[1, 0]]
    lg = torch.zeros((1, 1, 1, 2), device=dev, requires_grad=True)
    dl = torch.tensor([[[[1.0, 3.0]], [[-2.0, 3.0]], [[0.0, 3.0]], [[0.5, 3.0]]]], device=dev, requires_grad=True)
    out = rpn_loss.rpn_losses([lg], [dl], s, _cells_t(cells), [16], [torch.from_numpy(gts[0]).to(dev)], batch_size_per_image=2)
    assert abs(out["loss_rpn_cls"].item() - np.log(2.0)) <= 1e-6 and out["loss_rpn_loc"].item() == 1.75
    (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()
    assert lg.grad.reshape(-1).tolist() == [-0.25, 0.25]
    assert dl.grad.reshape(4, 2).tolist() == [[0.5, 0.0], [-0.5, 0.0], [0.0, 0.0], [0.5, 0.0]]
