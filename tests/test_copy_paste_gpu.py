"""unmore_amd.copy_paste on the device against the torch restatement (tests/copy_paste_common.py) and the reference's fixture."""
import numpy as np
import pytest
import torch

from copy_paste_common import blob_item, copy_paste_reference, load_fixture, resize_bytes_f32

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = (1, 63, 64, 65, 130), (1, 7, 48)
LABELED_SIZES = ((9, 70), (48, 64), (5, 3), (17, 129), (1, 1), (31, 33), (2, 65))
N_UNLABELED, N_COPY = (0, 1, 3, 9), (1, 2, 5)


def ragged_batch():
    """15 frames (every width x every height) with labeled sizes, instance counts, copy counts and placements cycling through their
    sets: ratio 1.0 at shift 0 (from a labeled item of the same size: the identity; and of another size), h_new = 1, both shift
    extremes; plus one pair with more copies and existing masks than one overlap tile holds."""
    rng = np.random.RandomState(7)
    labeled, unlabeled, params = [], [], []
    k = 0
    for Hu in HEIGHTS:
        for Wu in WIDTHS:
            Nu, nc = N_UNLABELED[k % 4], N_COPY[k % 3]
            variant = k % 5
            Hl, Wl = (Hu, Wu) if variant == 0 else LABELED_SIZES[k % len(LABELED_SIZES)]
            Nl = nc + (k % 2)
            if variant in (0, 1):                                   # ratio 1.0: the whole frame at shift 0
                ratio, h_new, w_new, h_shift, w_shift = 1.0, Hu, Wu, 0, 0
            elif variant == 2:                                      # one resized row, at the bottom right
                ratio = 1.5 / Hu if Hu > 1 else 1.0
                h_new, w_new = int(ratio * Hu), max(int(ratio * Wu), 1)
                h_shift, w_shift = Hu - h_new, Wu - w_new
            elif variant == 3:                                      # top left
                ratio = 0.6
                h_new, w_new, h_shift, w_shift = max(int(ratio * Hu), 1), max(int(ratio * Wu), 1), 0, 0
            else:                                                   # bottom right
                ratio = 0.77
                h_new, w_new = max(int(ratio * Hu), 1), max(int(ratio * Wu), 1)
                h_shift, w_shift = Hu - h_new, Wu - w_new
            labeled.append(blob_item(rng, Hl, Wl, Nl))
            unlabeled.append(blob_item(rng, Hu, Wu, Nu, empty=(2,) if k == 10 else ()))
            params.append((rng.permutation(Nl)[:nc].astype(np.int64), ratio, h_new, w_new, h_shift, w_shift))
            k += 1
    assert any(p[2] == 1 and p[0].size > 0 for p, u in zip(params, unlabeled) if u["image"].shape[1] > 1)
    labeled.append(blob_item(rng, 40, 50, 11))
    unlabeled.append(blob_item(rng, 37, 70, 10))
    params.append((rng.permutation(11)[:10].astype(np.int64), 0.5, 18, 35, 9, 20))
    labeled.append(blob_item(rng, 20, 20, 2))                       # a pair that does not copy, in the middle of the others' tables
    unlabeled.append(blob_item(rng, 21, 22, 2))
    params.append(None)
    order = rng.permutation(len(params))
    return [labeled[i] for i in order], [unlabeled[i] for i in order], [params[i] for i in order]


def to_dev(items):
    return [{k: v.cuda() for k, v in it.items()} for it in items]


@pytest.fixture(scope="module")
def ragged():
    from unmore_amd.copy_paste import copy_and_paste
    labeled, unlabeled, params = ragged_batch()
    ref = copy_paste_reference(labeled, unlabeled, params)
    ref_f32 = copy_paste_reference(labeled, unlabeled, params, image_resize=resize_bytes_f32)
    lab_d, unl_d = to_dev(labeled), to_dev(unlabeled)
    got = copy_and_paste(lab_d, unl_d, params)
    return dict(labeled=labeled, unlabeled=unlabeled, params=params, ref=ref, ref_f32=ref_f32, lab_d=lab_d, unl_d=unl_d, got=got)


def check_pair(g, r, r_f32, unl_d, tag):
    assert (g["image"] is unl_d["image"]) == r["unchanged"], tag                  # the keep decisions, as far as they show
    if r["unchanged"]:
        assert g["masks"] is unl_d["masks"] and g["boxes"] is unl_d["boxes"] and g["areas"] is None, tag
    else:
        assert g["masks"].dtype == torch.bool and g["boxes"].dtype == torch.float32 and g["image"].dtype == torch.uint8, tag
        assert torch.equal(g["areas"], r["masks"].sum((1, 2))), tag
    assert torch.equal(g["source"].cpu(), r["source"]), tag
    assert torch.equal(g["masks"].cpu().bool(), r["masks"].bool()), tag
    assert torch.equal(g["boxes"].cpu(), r["boxes"]), tag
    img = g["image"].cpu()
    if r_f32 is not None:
        assert torch.equal(img, r_f32["image"]), tag
    assert int((img.int() - r["image"].int()).abs().max()) <= 1, tag


def test_ragged_batch_equals_the_restatement(ragged):
    """One call over frames of width {1, 63, 64, 65, 130} x height {1, 7, 48}, N_u in {0, 1, 3, 9}, n_copy in {1, 2, 5} (and 10 copies on
    10 existing masks: several overlap tiles), labeled size != unlabeled size, ratio 1.0 at shift 0, h_new = 1, both shift extremes, an
    existing mask of area 0.  Masks, keep decisions, order, source, areas and boxes are exactly the restatement's; image bytes are exactly
    resize_bytes_f32 composited through the same alpha and within one level of F.interpolate's."""
    R = ragged
    assert len(R["got"]) == len(R["params"]) == 17
    kinds = {"unchanged": 0, "empty": 0, "dropped": 0, "rejected_some": 0}
    for p, (g, r, rf) in enumerate(zip(R["got"], R["ref"], R["ref_f32"])):
        check_pair(g, r, rf, R["unl_d"][p], f"pair {p}: params {R['params'][p]}")
        Nu = R["unlabeled"][p]["masks"].shape[0]
        kinds["unchanged"] += r["unchanged"]
        kinds["empty"] += (not r["unchanged"]) and Nu == 0
        if "areas" in r:
            kinds["dropped"] += bool((r["areas"] == 0).any())
            kinds["rejected_some"] += bool((~r["keep"]).any())
    print(kinds)
    assert kinds["unchanged"] >= 2 and kinds["empty"] >= 3 and kinds["rejected_some"] >= 1, kinds


def test_second_call_returns_identical_bytes(ragged):
    from unmore_amd.copy_paste import copy_and_paste
    R = ragged
    again = copy_and_paste(R["lab_d"], R["unl_d"], R["params"])
    for p, (a, b) in enumerate(zip(R["got"], again)):
        for key in ("image", "masks", "boxes", "source"):
            assert torch.equal(a[key], b[key]), (p, key)
    # and the inputs were not modified
    for d, h in zip(R["lab_d"] + R["unl_d"], R["labeled"] + R["unlabeled"]):
        for key in ("image", "masks", "boxes"):
            assert torch.equal(d[key].cpu(), h[key]), key


def test_fixture_batch_on_the_device():
    """Every branch of the reference's fixture batch (tests/golden/make_golden_copy_paste.py): image bytes within one level, everything
    else equal; unchanged items come back as the very input tensors."""
    from unmore_amd.copy_paste import copy_and_paste
    items, params, expected, _, _ = load_fixture()
    dev = to_dev(items)
    got = copy_and_paste(dev[::-1], dev, params)
    for p, (g, e) in enumerate(zip(got, expected)):
        assert (g["image"] is dev[p]["image"]) == e["unchanged"], p
        if e["unchanged"]:
            assert g["masks"] is dev[p]["masks"] and g["boxes"] is dev[p]["boxes"], p
        assert np.array_equal(g["masks"].cpu().numpy(), e["masks"]), p
        assert np.array_equal(g["boxes"].cpu().numpy(), e["boxes"]), p
        assert np.array_equal(g["source"].cpu().numpy(), e["source"]), p
        assert int(np.abs(g["image"].cpu().numpy().astype(np.int64) - e["image"].astype(np.int64)).max()) <= 1, p


def test_half_overlap_is_rejected_one_pixel_less_is_kept():
    """inter / area == 0.5 is not < 0.5: a copy covering exactly half of an existing mask is rejected, one pixel less and it is kept.
    Identity placement (same size, ratio 1.0, shift 0), so the pasted mask is the labeled mask; an existing mask of 2 x 65 pixels across
    a word boundary."""
    from unmore_amd.copy_paste import copy_and_paste
    H, W = 6, 130
    img = torch.arange(3 * H * W, dtype=torch.int64).remainder(251).to(torch.uint8).view(3, H, W)
    existing = torch.zeros(1, H, W, dtype=torch.bool)
    existing[0, 2:4, 30:95] = True                                  # area 130
    half = torch.zeros(2, H, W, dtype=torch.bool)
    half[0, 2, 30:95] = True                                        # 65 of 130
    half[1, 2, 30:94] = True                                        # 64 of 130
    boxes = torch.zeros(2, 4)
    lab = {"image": img.flip(2).contiguous(), "masks": half, "boxes": boxes}
    unl = {"image": img, "masks": existing, "boxes": torch.tensor([[30., 2., 95., 4.]])}
    prm = [(np.array([c]), 1.0, H, W, 0, 0) for c in (0, 1)]
    ref = copy_paste_reference([lab, lab], [unl, unl], prm)
    assert ref[0]["unchanged"] and not ref[1]["unchanged"]
    lab_d, unl_d = to_dev([lab])[0], to_dev([unl])[0]
    got = copy_and_paste([lab_d, lab_d], [unl_d, unl_d], prm)
    assert got[0]["image"] is unl_d["image"] and got[0]["masks"] is unl_d["masks"]
    check_pair(got[1], ref[1], None, unl_d, "one pixel less")
    assert got[1]["areas"].tolist() == [66, 64] and got[1]["source"].tolist() == [[0, 0], [1, 1]]
    assert torch.equal(got[1]["image"].cpu(), ref[1]["image"])      # the identity resize is exact


def test_drawn_params_and_cpu_tensors():
    """params=None draws from the global streams exactly as draw_params does; uint8 masks (0 / 255) are taken as they are; a CPU tensor
    is refused."""
    import random
    from unmore_amd.copy_paste import copy_and_paste, draw_params
    rng = np.random.RandomState(11)
    items = [blob_item(rng, 24, 40, 3), blob_item(rng, 30, 33, 0), blob_item(rng, 16, 70, 2)]
    items[0]["masks"] = items[0]["masks"].to(torch.uint8) * 255     # uint8 masks as rle.decode makes them: non-zero = set
    dev = to_dev(items)
    random.seed(4)
    np.random.seed(4)
    got = copy_and_paste(dev[::-1], dev)
    want = draw_params([it["masks"].shape[0] for it in items[::-1]], [it["image"].shape[1:] for it in items], 1.0, True, 0.3, 1.0,
                       py_random=random.Random(4), np_random=np.random.RandomState(4))
    ref = copy_paste_reference(items[::-1], items, want)
    for p, (g, w, r) in enumerate(zip(got, want, ref)):
        assert (g["params"] is None) == (w is None), p
        if w is not None:
            assert np.array_equal(g["params"][0], w[0]) and tuple(g["params"][1:]) == tuple(w[1:]), p
        check_pair(g, r, None, dev[p], f"pair {p}")
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        copy_and_paste([items[0]], [dev[0]], [None])
