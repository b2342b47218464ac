"""unmore_amd.mask_loss on the device against the NumPy / float64 restatement (tests/mask_loss_common.py) and the reference's fixture.

The batch (mask_loss_common.ragged_batch): frames of widths (1, 63, 64, 65, 130) x heights (1, 7, 48), 257 proposals with 0, 1, 3 or
40 per image, 1 or 5 masks per image, sides 7, 14 and 28 (28 puts more than one bin on a thread), boxes cycling through random float
boxes up to 3 px outside the frame, integer-aligned, sub-pixel, frame-sized (grid up to 19 at side 7), zero-width, negative-width and
fully outside ones, plus one NaN coordinate, one 1e9 coordinate and one mask index out of range.

Targets: a bin is DECIDED when the float64 restatement's average is more than 1e-5 from 0.5 -- at these sizes a bin sums at most 19^2
samples of four terms, and float32 then stays within about 1e-5 of float64 in the worst case (measured on this batch with the float32
restatement: below 4e-6, 19 of 264 453 bins undecided, no decided bin on which the two disagree).  Every decided bin must equal the
float64 decision; undecided bins may be at most 1 % of the bins compared.
Loss: 1e-5 * max(1, |loss64|) against the float64 restatement on the kernel's own targets -- per-element float32 error of a few ulp,
about log2(n) ulp from the fixed-order sum, a factor of five to spare.  Gradient: float32 logits 1e-5 relative + 1e-6 / (R M M)
absolute; bfloat16 logits one bfloat16 ulp of the float64 value."""
import numpy as np
import pytest
import torch

from mask_loss_common import load_fixture, logged_scalars, loss_reference, mask_averages_np, mask_targets_np, ragged_batch

pytestmark = pytest.mark.gpu

SIDES = {7: 1, 14: 3, 28: 1}                      # side -> channels of the logits


KEYS = {"masks": "gt_masks", "boxes": "proposal_boxes", "mask_index": "mask_index", "gt_classes": "gt_classes"}


def to_dev(images):
    return [{KEYS[k]: torch.from_numpy(v).cuda() for k, v in im.items()} for im in images]


def call(images, logits, weights, **kw):
    """one fused call with its backward: (loss, gradient, stats), all still on the device"""
    from unmore_amd.mask_loss import mask_rcnn_loss_weighted
    x = logits.clone().requires_grad_(True)
    stats = {}
    loss = mask_rcnn_loss_weighted(x, images, weights, stats=stats, **kw)
    loss.backward()
    return loss.detach(), x.grad, stats


class Case:
    def __init__(self, side, C):
        self.side, self.C = side, C
        self.images, self.logits, self.weights, self.n_bad = ragged_batch(side, C)
        self.classes = np.concatenate([im["gt_classes"] for im in self.images])
        avg = [mask_averages_np(im["masks"], im["boxes"], im["mask_index"], side, np.float64) for im in self.images]
        self.avg64 = np.concatenate([a for a, _ in avg])
        self.bad = np.concatenate([b for _, b in avg])
        self.t32 = np.concatenate([mask_targets_np(im["masks"], im["boxes"], im["mask_index"], side, np.float32) for im in self.images])
        self.dev = to_dev(self.images)
        self.x, self.w = torch.from_numpy(self.logits).cuda(), torch.from_numpy(self.weights).cuda()
        self.loss, self.grad, self.stats = call(self.dev, self.x, self.w)
        self.targets = self.stats["targets"].cpu().numpy()
        self.counters = self.stats["counters"].cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    return {side: Case(side, C) for side, C in SIDES.items()}


@pytest.mark.parametrize("side", sorted(SIDES))
def test_targets_equal_the_float64_decision_on_every_decided_bin(cases, side):
    c = cases[side]
    assert c.targets.shape == c.avg64.shape == (257, side, side) and c.targets.dtype == bool
    undecided = np.abs(c.avg64 - 0.5) <= 1e-5
    print(f"side {side}: {int(undecided.sum())} of {undecided.size} bins undecided; "
          f"{int((c.targets != c.t32)[undecided].sum())} of them differ from the float32 restatement, "
          f"{int((c.targets != c.t32).sum())} bins differ from it in all")
    assert undecided.sum() <= 0.01 * undecided.size
    assert np.array_equal(c.targets[~undecided], (c.avg64 >= 0.5)[~undecided])
    assert 0.02 < c.targets.mean() < 0.9                                   # the batch has both kinds of bins
    assert not c.targets[c.bad].any() and c.bad.sum() == c.n_bad


@pytest.mark.parametrize("side", sorted(SIDES))
def test_loss_and_counters(cases, side):
    c = cases[side]
    loss64, counters64, _ = loss_reference(c.logits, c.targets, c.classes, c.weights)
    got = float(c.loss)
    print(f"side {side}: loss {got!r}, float64 {loss64!r}, difference {abs(got - loss64):.3e}; counters {c.counters.tolist()}")
    assert c.loss.dtype == torch.float32 and c.loss.dim() == 0
    assert abs(got - loss64) <= 1e-5 * max(1.0, abs(loss64))
    assert np.array_equal(c.counters[:4], counters64)
    assert c.counters[4] == c.n_bad
    s = c.stats["scalars"]()
    want = logged_scalars(counters64, c.targets.size)
    assert s["bad"] == c.n_bad and all(abs(s[k] - want[k]) <= 1e-12 for k in want)
    assert s == c.stats["scalars"](c.counters)


@pytest.mark.parametrize("side", sorted(SIDES))
def test_gradient_float32(cases, side):
    c = cases[side]
    _, _, g64 = loss_reference(c.logits, c.targets, c.classes, c.weights)
    g = c.grad.cpu().numpy().astype(np.float64)
    n = c.targets.size
    err = np.abs(g - g64) - (1e-5 * np.abs(g64) + 1e-6 / n)
    print(f"side {side}: largest gradient error over its bound {err.max():.3e} (bound at that element "
          f"{(1e-5 * np.abs(g64) + 1e-6 / n).flat[err.argmax()]:.3e})")
    assert c.grad.dtype == torch.float32 and err.max() <= 0
    if c.C > 1:
        other = np.ones(g.shape, dtype=bool)
        other[np.arange(len(c.classes)), c.classes] = False
        assert not g[other].any() and g[~other].any()


@pytest.mark.parametrize("side", (14, 28))
def test_bfloat16_logits(cases, side):
    """Loss and counters from the bfloat16 values in float32 arithmetic; gradient within one bfloat16 ulp of float64."""
    c = cases[side]
    xb = c.x.bfloat16()
    loss, grad, stats = call(c.dev, xb, c.w)
    targets = stats["targets"].cpu().numpy()
    assert np.array_equal(targets, c.targets)
    loss64, counters64, g64 = loss_reference(xb.float().cpu().numpy(), targets, c.classes, c.weights)
    assert abs(float(loss) - loss64) <= 1e-5 * max(1.0, abs(loss64))
    assert np.array_equal(stats["counters"].cpu().numpy()[:4], counters64)
    assert grad.dtype == torch.bfloat16
    g = grad.float().cpu().numpy().astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(g64), 1e-300))) - 7)
    print(f"side {side}: largest bfloat16 gradient error {np.max(np.abs(g - g64) / ulp):.3f} ulp")
    assert (np.abs(g - g64) <= ulp).all()
    assert not g[g64 == 0].any()


def test_backward_scales_the_saved_gradient(cases):
    from unmore_amd.mask_loss import mask_rcnn_loss_weighted
    c = cases[14]
    x = c.x.clone().requires_grad_(True)
    (0.37 * mask_rcnn_loss_weighted(x, c.dev, c.w)).backward()
    assert torch.allclose(x.grad, 0.37 * c.grad, rtol=1e-6, atol=0)
    assert x.grad.abs().max() > 0


def test_no_proposals():
    """R == 0: a zero loss that is still attached to the graph, a zero gradient."""
    from unmore_amd.mask_loss import mask_rcnn_loss_weighted
    rng = np.random.RandomState(0)
    images, _, _, _ = ragged_batch(7, 1)
    empty = to_dev([im for im in images if im["boxes"].shape[0] == 0])
    assert len(empty) == 2
    for instances in (empty, []):
        x = torch.from_numpy(rng.standard_normal((0, 1, 7, 7)).astype(np.float32)).cuda().requires_grad_(True)
        stats = {}
        loss = mask_rcnn_loss_weighted(x, instances, torch.zeros(0, device="cuda"), stats=stats)
        assert loss.item() == 0.0 and loss.requires_grad and loss.grad_fn is not None and loss.dtype == torch.float32
        loss.backward()
        assert x.grad is not None and x.grad.shape == x.shape
        assert stats["counters"].tolist() == [0, 0, 0, 0, 0] and stats["scalars"]()["accuracy"] == 1.0
    # part of a larger graph, as the head's loss dict is summed
    y = torch.ones(3, device="cuda", requires_grad=True)
    x = torch.zeros(0, 2, 7, 7, device="cuda", requires_grad=True)
    total = y.sum() + mask_rcnn_loss_weighted(x, [], None)
    total.backward()
    assert y.grad.tolist() == [1.0, 1.0, 1.0]


def test_hand_worked_targets_on_the_device():
    """The dyadic cases of tests/test_mask_loss_cpu.py: every bin must match."""
    from unmore_amd.mask_loss import mask_targets
    for M in (4, 7, 28):
        rng = np.random.RandomState(M)
        H, W = 3 * M + 5, 3 * M + 2
        mask = rng.rand(H, W) < 0.5
        y0, x0 = 3, 2
        boxes = np.array([[x0, y0, x0 + M, y0 + M], [x0, y0, x0 + 2 * M, y0 + 2 * M], [W + 2, 0, W + 2 + M, M], [0, -M - 3, M, -3],
                          [-3 * M, -3 * M, -M, -M], [4, 4, 4, 4 + M], [4 + M, 4, 4, 4 + M], [4, 9, 4 + M, 5]], dtype=np.float32)
        got = mask_targets(torch.from_numpy(mask[None]).cuda(), torch.from_numpy(boxes).cuda(), torch.zeros(8, dtype=torch.int32).cuda(), M)
        got = got.cpu().numpy()
        assert np.array_equal(got[0], mask[y0:y0 + M, x0:x0 + M])
        assert np.array_equal(got[1], mask[y0:y0 + 2 * M, x0:x0 + 2 * M].reshape(M, 2, M, 2).sum((1, 3)) >= 2)
        assert not got[2:].any()
        assert np.array_equal(got, mask_targets_np(mask[None], boxes, np.zeros(8, dtype=np.int64), M, np.float32))
    one = torch.ones(1, 1, 1, dtype=torch.bool).cuda()
    boxes = torch.tensor([[-0.5, -0.5, 1.5, 1.5]]).cuda()
    assert mask_targets(one, boxes, None, 2).all()
    assert not mask_targets(~one, boxes, None, 2).any()
    # a quarter of bin 0's samples lie inside [-1, 1]: 0.25 < 0.5; with a box half as wide it is a half, an exact tie, and counts
    assert not mask_targets(one, torch.tensor([[-3.5, -0.5, 12.5, 1.5]]).cuda(), None, 2).any()
    got = mask_targets(one, torch.tensor([[-1.5, -0.5, 6.5, 1.5]]).cuda(), None, 2).cpu().numpy()[0]
    assert np.array_equal(got, np.array([[True, False], [True, False]]))


def test_a_box_of_absurd_size_is_bounded_work():
    """A box of 2^20 pixels per side is allowed: its grid has 10^5 samples per bin and axis, of which the kernel walks only those inside
    the frame.  The frame lies in bin 0 of each axis, where 65 x 48 of the 149797 x 149797 samples hit a set pixel: a zero target; over
    a 2 M x 2 M integer box at the origin the all-ones mask gives ones."""
    from unmore_amd.mask_loss import mask_targets
    ones = torch.ones(1, 48, 65, dtype=torch.bool).cuda()
    boxes = torch.tensor([[0.0, 0.0, 1048576.0, 1048576.0], [-1048576.0, -1048576.0, 1048576.0, 1048576.0], [0.0, 0.0, 14.0, 14.0]]).cuda()
    got = mask_targets(ones, boxes, torch.zeros(3, dtype=torch.int64).cuda(), 7).cpu().numpy()
    assert not got[0].any() and not got[1].any() and got[2].all()


@pytest.mark.parametrize("side", (28, 33))
def test_large_proposals_shared_by_workgroups(side):
    """A proposal of more than 65536 samples is shared by ceil(side^2 / 256) workgroups, whole rows of bins each (side 28: 4 x 7 rows;
    side 33: 5 workgroups of 7, 7, 7, 7, 5 rows).  A 300 x 400 frame: the frame-sized box (308 x 420 samples at side 28), boxes just
    below and just above the threshold (280 x 224 and 308 x 224 at side 28), a box reaching 5000 px outside, a small one, a bad index."""
    rng = np.random.RandomState(side)
    H, W, G = 300, 400, 2
    from mask_loss_common import blob_masks
    masks = blob_masks(rng, H, W, G, 0.2, 0.5)
    boxes = np.array([[0, 0, W, H], [0.3, 0.2, 280.3, 224.2], [0.3, 0.2, 300.3, 224.2], [150.5, 100.25, 5000, 290], [30, 40, 70, 90],
                      [0, 0, W, H], [-40.5, -30.25, W + 20.5, H + 33.75]], dtype=np.float32)
    idx = np.array([0, 1, 0, 1, 0, G, 1], dtype=np.int64)
    R = len(boxes)
    logits = (rng.standard_normal((R, 1, side, side)) * 3).astype(np.float32)
    weights = rng.uniform(0.1, 2.0, size=R).astype(np.float32)
    dev = [{"gt_masks": torch.from_numpy(masks).cuda(), "proposal_boxes": torch.from_numpy(boxes).cuda(), "mask_index": torch.from_numpy(idx).cuda()}]
    loss, grad, stats = call(dev, torch.from_numpy(logits).cuda(), torch.from_numpy(weights).cuda())
    targets = stats["targets"].cpu().numpy()
    avg64 = mask_averages_np(masks, boxes, idx, side, np.float64)[0]
    t32 = mask_targets_np(masks, boxes, idx, side, np.float32)
    undecided = np.abs(avg64 - 0.5) <= 1e-5
    print(f"side {side}: {int(undecided.sum())} of {undecided.size} bins undecided, {int((targets != t32).sum())} bins differ from the float32 "
          f"restatement")
    assert undecided.sum() <= 0.01 * undecided.size
    assert np.array_equal(targets[~undecided], (avg64 >= 0.5)[~undecided])
    assert 0.1 < targets[:5].mean() < 0.9 and not targets[5].any()
    loss64, counters64, g64 = loss_reference(logits, targets, None, weights)
    assert abs(loss.item() - loss64) <= 1e-5 * max(1.0, abs(loss64))
    assert stats["counters"].tolist() == counters64.tolist() + [1]
    g = grad.cpu().numpy().astype(np.float64)
    assert (np.abs(g - g64) <= 1e-5 * np.abs(g64) + 1e-6 / targets.size).all()
    from unmore_amd.mask_loss import mask_targets
    assert torch.equal(mask_targets(dev[0]["gt_masks"], dev[0]["proposal_boxes"], dev[0]["mask_index"], side), stats["targets"])


def test_fixture_on_the_device():
    from unmore_amd.mask_loss import mask_rcnn_loss
    fx = load_fixture()
    dev = to_dev(fx["images"])
    n = fx["targets"].size
    classes = np.concatenate([im["gt_classes"] for im in fx["images"]])
    for name, case in fx["cases"].items():
        x = torch.from_numpy(case["logits"]).cuda()
        if case["weighted"]:
            loss, grad, stats = call(dev, x, torch.from_numpy(fx["weights"]).cuda())
        else:
            xr = x.clone().requires_grad_(True)
            stats = {}
            loss = mask_rcnn_loss(xr, dev, stats=stats)
            loss.backward()
            grad = xr.grad
        assert abs(loss.item() - case["loss"]) <= 1e-5 * abs(case["loss"]), name
        targets = stats["targets"].cpu().numpy()
        avg64 = np.concatenate([mask_averages_np(im["masks"], im["boxes"], im["mask_index"], fx["side"], np.float64)[0] for im in fx["images"]])
        decided = np.abs(avg64 - 0.5) > 1e-5
        assert decided.mean() >= 0.99 and np.array_equal(targets[decided], fx["targets"][decided]), name
        s = stats["scalars"]()
        same = np.array_equal(targets, fx["targets"])                       # the 12 exact ties of the fixture included
        print(f"{name}: loss {loss.item()!r}, fixture {case['loss']!r}; targets equal to the fixture's on every bin: {same}")
        if same:
            assert np.allclose([s["accuracy"], s["false_positive"], s["false_negative"]], case["scalars"], rtol=1e-12, atol=0), name
            assert np.abs(grad.cpu().numpy() - case["grad"]).max() <= 1e-5 * np.abs(case["grad"]).max(), name
        _, _, g64 = loss_reference(case["logits"], targets, classes, fx["weights"] if case["weighted"] else None)
        g = grad.cpu().numpy().astype(np.float64)
        assert (np.abs(g - g64) <= 1e-5 * np.abs(g64) + 1e-6 / n).all(), name
        assert s["bad"] == 0


def test_two_calls_give_the_same_bytes(cases):
    c = cases[28]
    loss, grad, stats = call(c.dev, c.x, c.w)
    assert torch.equal(loss.view(torch.int32), c.loss.view(torch.int32))
    assert torch.equal(grad.view(torch.int32), c.grad.view(torch.int32))
    assert torch.equal(stats["counters"], c.stats["counters"]) and torch.equal(stats["targets"], c.stats["targets"])


def test_mask_targets_alone_equal_the_fused_call(cases):
    from unmore_amd.mask_loss import mask_targets
    for side, c in cases.items():
        got = mask_targets([im["gt_masks"] for im in c.dev], [im["proposal_boxes"] for im in c.dev], [im["mask_index"] for im in c.dev], side)
        assert got.dtype == torch.bool and torch.equal(got, c.stats["targets"]), side
    c = cases[7]
    k = 3                                                                   # one image on its own, 40 proposals
    first = sum(im["boxes"].shape[0] for im in c.images[:k])
    got = mask_targets(c.dev[k]["gt_masks"], c.dev[k]["proposal_boxes"], c.dev[k]["mask_index"], 7)
    assert torch.equal(got, c.stats["targets"][first:first + 40])


def test_weights_none_is_weights_of_ones(cases):
    c = cases[14]
    a = call(c.dev, c.x, None)
    b = call(c.dev, c.x, torch.ones_like(c.w))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2]["counters"], b[2]["counters"])
    assert float(a[0]) != float(c.loss)
