"""unmore_amd.detector_input on the device against the host form (tests/det_input_common.py) and the reference's fixture
(tests/golden/det_input.npz).  Every comparison is for equality: PIL's 8-bit resize is integer arithmetic, the nearest resize a table
lookup, the normalisation one float32 subtract and one float32 divide."""
import numpy as np
import pytest
import torch

import det_input_common as C

pytestmark = pytest.mark.gpu

N_MASKS = (0, 1, 3, 9)


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch of C.resize_cases(): seeded noise images, N in (0, 1, 3, 9) blob / noise masks each, and the host form's answers"""
    rng = np.random.RandomState(11)
    cases = C.resize_cases()
    images = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W, _, _, _ in cases]
    masks = [rng.rand(N_MASKS[i % 4], c[0], c[1]) < 0.15 for i, c in enumerate(cases)]
    want_img = [C.flip_last(C.resize_bilinear(im, nh, nw).transpose(2, 0, 1), f) for im, (_, _, nh, nw, f) in zip(images, cases)]
    want_msk = [C.flip_last(C.resize_nearest(m, nh, nw), f) for m, (_, _, nh, nw, f) in zip(masks, cases)]
    return dict(cases=cases, images=images, masks=masks, want_img=want_img, want_msk=want_msk)


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


def test_bilinear_ragged_batch_equals_the_host_form(ragged):
    """One call over widths {1, 63, 64, 65, 130, 131} x heights {1, 7, 48}: upscale, mild and extreme downscale (131 -> 10), identity in
    one axis and in both, outputs one below / at / above the tile edges, with and without the horizontal flip, the vertical flip once,
    3 -> 40, and the two shapes whose staged rows need a lower tile (400 -> 40 rows) and a narrower one (700 -> 4 rows).  Device inputs; then
    the same batch from the host in the call's one copy; the inputs are unchanged."""
    from unmore_amd import detector_input as D
    R = ragged
    shapes, flips = [c[2:4] for c in R["cases"]], [c[4] for c in R["cases"]]
    tiles = {D.tile_shape(*D.bilinear_table(c[0], c[2])[:2], c[2]) for c in R["cases"]}
    assert tiles == {(32, 64), (16, 64), (1, 16)}, tiles           # the full tile, the lower one (400 -> 40 rows), the narrower one (700 -> 4)
    assert sum(f == C.FLIP_V for f in flips) == 1 and sum(f == C.FLIP_H for f in flips) > 10 and sum(f == 0 for f in flips) > 10
    assert any(c[:2] == c[2:4] for c in R["cases"]) and {c[4] for c in R["cases"] if c[1] == 131 and c[3] == 10} == {C.FLIP_NONE, C.FLIP_H}
    host = [torch.from_numpy(im) for im in R["images"]]
    dev = [t.cuda() for t in host]
    got = D.resize_images(dev, shapes, flips)
    for i, (g, w) in enumerate(zip(got, R["want_img"])):
        assert g.dtype == torch.uint8 and g.is_cuda and tuple(g.shape) == w.shape, R["cases"][i]
        assert np.array_equal(g.cpu().numpy(), w), R["cases"][i]
    again = D.resize_images(host, [(nh, nw, f) for (nh, nw), f in zip(shapes, flips)])          # host inputs, triples
    for i, (g, w) in enumerate(zip(again, R["want_img"])):
        assert np.array_equal(g.cpu().numpy(), w), R["cases"][i]
    mixed = D.resize_images([host[0], dev[1], host[2]], shapes[:3], [bool(f) for f in flips[:3]])
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(mixed, R["want_img"]))
    for d, h, im in zip(dev, host, R["images"]):
        assert np.array_equal(d.cpu().numpy(), im) and np.array_equal(h.numpy(), im)


def test_masks_ragged_batch_equals_the_host_form(ragged):
    """the same shapes with N in (0, 1, 3, 9) masks per image, as bool and as 0 / 255 uint8 (what rle.decode writes); the non-empty flags"""
    from unmore_amd import detector_input as D
    R = ragged
    shapes, flips = [c[2:4] for c in R["cases"]], [c[4] for c in R["cases"]]
    assert {m.shape[0] for m in R["masks"]} == set(N_MASKS)
    as_bool = [torch.from_numpy(m).cuda() for m in R["masks"]]
    as_u8 = [torch.from_numpy(m.astype(np.uint8) * 255).cuda() for m in R["masks"]]
    for inputs in (as_bool, as_u8, [torch.from_numpy(m) for m in R["masks"]]):
        got, flags = D.resize_masks(inputs, shapes, flips)
        for i, (g, f, w) in enumerate(zip(got, flags, R["want_msk"])):
            assert g.dtype == torch.bool and f.dtype == torch.bool and g.is_cuda and tuple(g.shape) == w.shape, R["cases"][i]
            assert np.array_equal(g.cpu().numpy(), w), R["cases"][i]
            assert np.array_equal(f.cpu().numpy(), w.any(axis=(1, 2))), R["cases"][i]
    assert any(not w.any(axis=(1, 2)).all() for w in R["want_msk"] if w.shape[0]) and any(w.any() for w in R["want_msk"])
    for d, m in zip(as_bool, R["masks"]):
        assert np.array_equal(d.cpu().numpy(), m)


def test_masks_repeated_addition_pair_and_one_pixel_masks():
    """The size pair whose repeated-addition table differs from (i + 0.5) * a (tests/test_det_input_cpu.py finds it): the device follows
    the addition.  A one-pixel mask the sampling misses has its flag false, one it hits true; rle.decode's output feeds the call."""
    from unmore_amd import detector_input as D
    from unmore_amd import rle
    inn, out = C.NEAREST_PAIR
    m = np.stack([np.arange(inn) % 2, np.arange(inn) % 3 == 0]).astype(bool)[None]             # [1, 2, in]: two rows
    add, mul = C.nearest_table(inn, out), C.nearest_table_mul(inn, out)
    assert not np.array_equal(m[..., add], m[..., mul])
    H, W, nh, nw = 40, 60, 17, 23
    ty, tx = C.nearest_table(H, nh), C.nearest_table(W, nw)
    miss_y = next(v for v in range(H) if v not in set(ty.tolist()))
    one = np.zeros((2, H, W), dtype=np.uint8)
    one[0, miss_y, int(tx[5])] = 1                                   # a row the table skips
    one[1, int(ty[9]), int(tx[5])] = 1                               # a pixel it samples
    decoded = rle.decode([rle.encode_numpy(one[0]), rle.encode_numpy(one[1])])                # 0 / 255, each mask 16-byte aligned
    stack = torch.stack(decoded)
    got, flags = D.resize_masks([torch.from_numpy(m).cuda(), stack, torch.from_numpy(m[:, :, ::-1].copy())], [(2, out), (nh, nw), (2, out)],
                                [0, 1, 0])
    assert np.array_equal(got[0].cpu().numpy(), m[..., add]) and np.array_equal(got[2].cpu().numpy(), m[:, :, ::-1][..., add])
    want = C.flip_last(C.resize_nearest(one != 0, nh, nw), C.FLIP_H)
    assert np.array_equal(got[1].cpu().numpy(), want) and want[1].sum() == 1 and not want[0].any()
    assert flags[1].tolist() == [False, True] and flags[0].tolist() == [True]
    assert torch.equal(stack, torch.stack(decoded)) and int(stack.max()) == 255


def _to_tensors(fx, device_images):
    imgs = [torch.from_numpy(im) for im in fx["images"]]
    return [t.cuda() for t in imgs] if device_images else imgs


def _check_item(g, e, k, padded=False):
    assert np.array_equal(g["image"].cpu().numpy(), e["image"]), k
    sel = g["keep"].cpu().numpy() if padded else slice(None)
    if padded:
        assert np.array_equal(sel, e["keep"]), k
    for key in ("masks", "boxes", "scores", "classes"):
        got = g[key].cpu().numpy()[sel]
        assert got.dtype == e[key].dtype and got.shape == e[key].shape, (k, key)
        assert np.array_equal(got.view(np.uint8), e[key].view(np.uint8)), (k, key)                # bits, not values
    assert np.array_equal(g["source"].cpu().numpy()[sel], e["source"]) and g["source"].dtype == torch.int64, k
    assert (g["height"], g["width"], g["is_single_object"]) == (e["height"], e["width"], e["is_single_object"]), k


@pytest.mark.parametrize("device_images", [True, False])
def test_map_batch_equals_the_reference_fixture(fx, device_images):
    """list form and padded form, `source`, an image without annotations, one that loses every instance, run-length records decoded
    inside the call, host and device images; drawn transforms (the global stream) equal the reference's draws; inputs unchanged"""
    from unmore_amd import detector_input as D
    cfg = fx["cfg"]
    imgs = _to_tensors(fx, device_images)
    transforms = [d[1:] for d in fx["draws"]]
    got = D.map_batch(imgs, fx["annotations"], transforms, image_ids=fx["image_ids"])
    assert len(got) == len(fx["expected"])
    for k, (g, e) in enumerate(zip(got, fx["expected"])):
        _check_item(g, e, k)
        assert all(g[key].is_cuda for key in ("image", "masks", "boxes", "scores", "classes", "source")), k
    assert any(g["masks"].shape[0] == 0 and len(a) == 0 for g, a in zip(got, fx["annotations"]))
    assert any(g["masks"].shape[0] == 0 and len(a) > 0 for g, a in zip(got, fx["annotations"]))
    pad = D.map_batch(imgs, fx["annotations"], transforms, image_ids=fx["image_ids"], padded=True)
    for k, (g, e, a) in enumerate(zip(pad, fx["expected"], fx["annotations"])):
        assert g["masks"].shape[0] == sum(o["iscrowd"] == 0 for o in a) == g["keep"].shape[0], k
        _check_item(g, e, k, padded=True)
        assert g["rle_status"] is None or not bool(g["rle_status"].any()), k
    np.random.seed(cfg["seed"])
    drawn = D.map_batch(imgs, fx["annotations"], min_size=cfg["min_size"], max_size=cfg["max_size"], image_ids=fx["image_ids"])
    for k, (g, e) in enumerate(zip(drawn, fx["expected"])):
        _check_item(g, e, k)
    for t, im in zip(imgs, fx["images"]):
        assert np.array_equal(t.cpu().numpy(), im)


def test_map_batch_at_test_time_and_decoded_segmentations(fx):
    """is_train=False: no flip, the original height / width, no annotations needed.  Segmentations given as decoded masks -- host arrays
    (they join the upload), device tensors, and mixed with records -- give what the records give."""
    from unmore_amd import detector_input as D
    from unmore_amd import rle
    cfg = fx["cfg"]
    imgs = _to_tensors(fx, True)
    got = D.map_batch(imgs, None, is_train=False, min_size=cfg["min_size_test"], max_size=cfg["max_size_test"],
                      np_random=np.random.RandomState(cfg["seed"] + 1))
    for k, (g, e) in enumerate(zip(got, fx["expected_test"])):
        assert sorted(g) == ["height", "image", "width"], k
        assert np.array_equal(g["image"].cpu().numpy(), e["image"]) and (g["height"], g["width"]) == (e["height"], e["width"]), k
    transforms = [d[1:] for d in fx["draws"]]
    variants = []
    for k, annos in enumerate(fx["annotations"]):
        out = []
        for j, a in enumerate(annos):
            m = rle.decode_numpy(a["segmentation"])
            kind = (k + (j if k == 0 else 0)) % 3                    # image 0 mixes the three forms
            seg = m * 255 if kind == 0 else torch.from_numpy(m.astype(bool)).cuda() if kind == 1 else a["segmentation"]
            out.append(dict(a, segmentation=seg))
        variants.append(out)
    got = D.map_batch(imgs, variants, transforms, image_ids=fx["image_ids"])
    for k, (g, e) in enumerate(zip(got, fx["expected"])):
        _check_item(g, e, k)


def test_map_batch_reads_mask_stacks_in_place_and_sends_large_host_inputs_directly(fx, monkeypatch):
    """Decoded masks that are the slices of one tensor are read in place on the device (rle.decode's 16-byte aligned views too) and go up
    in one copy from the host; with the size threshold lowered, host images and mask stacks take the direct-copy path the full-size
    batches take.  The answers do not change."""
    from unmore_amd import detector_input as D
    from unmore_amd import rle
    monkeypatch.setattr(D, "DIRECT_BYTES", 1)
    variants = []
    for k, annos in enumerate(fx["annotations"]):
        if not annos:
            variants.append([])
            continue
        if k % 3 == 0:
            stack = rle.decode([a["segmentation"] for a in annos])                               # device views, one aligned stride apart
        else:
            stack = torch.from_numpy(np.stack([rle.decode_numpy(a["segmentation"]) for a in annos]).astype(bool))
            stack = stack.cuda() if k % 3 == 1 else stack
        variants.append([dict(a, segmentation=stack[j]) for j, a in enumerate(annos)])
    assert {len(v) and (v[0]["segmentation"].is_cuda, v[0]["segmentation"].dtype) for v in variants} >= {
        (True, torch.uint8), (True, torch.bool), (False, torch.bool)}
    got = D.map_batch(_to_tensors(fx, False), variants, [d[1:] for d in fx["draws"]], image_ids=fx["image_ids"])
    for k, (g, e) in enumerate(zip(got, fx["expected"])):
        _check_item(g, e, k)


def test_map_batch_feeds_copy_and_paste_and_preprocess_image(fx):
    """map_batch's items go through copy_and_paste and preprocess_image without conversion; the normalised batch of the mapped items
    is the reference's (GeneralizedRCNN.preprocess_image on the reference mapper's outputs)"""
    from unmore_amd import detector_input as D
    from unmore_amd.copy_paste import copy_and_paste, draw_params
    import random
    cfg = fx["cfg"]
    items = D.map_batch(_to_tensors(fx, False), fx["annotations"], [d[1:] for d in fx["draws"]], image_ids=fx["image_ids"])
    batch, sizes = D.preprocess_image(items, cfg["pixel_mean"], cfg["pixel_std"], cfg["size_divisibility"])
    assert batch.dtype == torch.float32 and tuple(batch.shape) == fx["batch"].shape and sizes == fx["image_sizes"]
    assert np.array_equal(batch.cpu().numpy().view(np.uint32), fx["batch"].view(np.uint32))
    params = draw_params([it["masks"].shape[0] for it in items[::-1]], [it["image"].shape[1:] for it in items], 1.0, True, 0.3, 1.0,
                         py_random=random.Random(3), np_random=np.random.RandomState(3))
    pasted = copy_and_paste(items[::-1], items, params)
    assert len(pasted) == len(items) and any(p["image"] is not it["image"] for p, it in zip(pasted, items))
    from copy_paste_common import copy_paste_reference
    host = [{k: it[k].cpu() for k in ("image", "masks", "boxes")} for it in items]
    ref = copy_paste_reference(host[::-1], host, params)
    for p, r in zip(pasted, ref):
        assert torch.equal(p["masks"].cpu().bool(), r["masks"].bool()) and torch.equal(p["boxes"].cpu(), r["boxes"])
    batch2, sizes2 = D.preprocess_image(pasted, cfg["pixel_mean"], cfg["pixel_std"], cfg["size_divisibility"])
    want, wsizes = C.normalize_pad([p["image"].cpu().numpy() for p in pasted], cfg["pixel_mean"], cfg["pixel_std"], cfg["size_divisibility"])
    assert sizes2 == wsizes and np.array_equal(batch2.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def norm_images():
    rng = np.random.RandomState(5)
    return [torch.from_numpy(rng.randint(0, 256, (3, h, w)).astype(np.uint8)) for h, w in ((1, 1), (31, 33), (32, 64), (65, 130))]


def _torch_reference(images, mean, std, div, pad):
    """torch CPU (x - mean) / std in float32, placed in a tensor of pad_value"""
    mean, std = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1), torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    Hp, Wp = max(im.shape[1] for im in images), max(im.shape[2] for im in images)
    if div > 1:
        Hp, Wp = (Hp + div - 1) // div * div, (Wp + div - 1) // div * div
    out = torch.full((len(images), 3, Hp, Wp), pad, dtype=torch.float32)
    for b, im in enumerate(images):
        out[b, :, :im.shape[1], :im.shape[2]] = (im - mean) / std
    return out


@pytest.mark.parametrize("div", [0, 1, 32])
@pytest.mark.parametrize("pad", [0.0, -1.5])
def test_preprocess_image_equals_torch(norm_images, div, pad):
    """sizes {1x1, 31x33, 32x64, 65x130} as one batch, every image alone (B = 1; 32x64 is already a multiple of 32), size_divisibility
    0 / 1 / 32, a non-zero pad value; bit for bit torch's float32 (x - mean) / std; bare tensors and dicts"""
    from unmore_amd import detector_input as D
    mean, std = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]
    dev = [im.cuda() for im in norm_images]
    for batch in [dev] + [[d] for d in dev]:
        host = [b.cpu() for b in batch]
        want = _torch_reference(host, mean, std, div, pad)
        got, sizes = D.preprocess_image(batch if len(batch) > 1 else [{"image": batch[0]}], mean, std, div, pad)
        assert got.dtype == torch.float32 and got.shape == want.shape and sizes == [tuple(im.shape[1:]) for im in host]
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (div, pad, [tuple(b.shape) for b in batch])
    if div == 32:
        assert tuple(D.preprocess_image([dev[2]], mean, std, 32)[0].shape) == (1, 3, 32, 64)
    for d, h in zip(dev, norm_images):
        assert torch.equal(d.cpu(), h)


def test_argument_errors_raise_before_any_launch(fx):
    """wrong dtype / layout, zero sizes, a mask whose size differs from its image, a transform whose shape is not positive, a score on
    some annotations only, polygons: ValueError naming the image and field, and the library's launch counter has not moved; tensors off
    the GPU where the GPU is required: RuntimeError"""
    from unmore_amd import _lib as L
    from unmore_amd import detector_input as D
    L.lib()
    img = torch.zeros((8, 9, 3), dtype=torch.uint8).cuda()
    ann = {"bbox": [1.0, 1.0, 3.0, 3.0], "bbox_mode": D.XYWH_ABS, "segmentation": torch.ones((8, 9), dtype=torch.bool).cuda()}
    t = [(8, 9, 0)]
    before = L._count[0]
    bad_calls = [
        ("images\\[1\\]", lambda: D.map_batch([img, img.float()], [[ann], [ann]], t * 2)),
        ("images\\[0\\]", lambda: D.resize_images([img.permute(2, 0, 1)], [(4, 4)], [0])),
        ("images\\[0\\]", lambda: D.resize_images([img[:0]], [(4, 4)], [0])),
        ("transforms\\[0\\]", lambda: D.map_batch([img], [[ann]], [(8, 0, 0)])),
        ("annotations\\[0\\]\\[0\\].*size", lambda: D.map_batch([img], [[dict(ann, segmentation=torch.ones((9, 8), dtype=torch.bool).cuda())]], t)),
        ("annotations\\[0\\]\\[1\\].*polygon", lambda: D.map_batch([img], [[ann, dict(ann, segmentation=[[1, 1, 4, 1, 4, 4]])]], t)),
        ("annotations\\[0\\].*score", lambda: D.map_batch([img], [[dict(ann, score=0.5), ann]], t)),
        ("masks\\[0\\]", lambda: D.resize_masks([torch.zeros((2, 8, 9)).cuda()], [(4, 4)], [0])),
        ("images\\[0\\]", lambda: D.preprocess_image([img], [1., 2., 3.], [1., 1., 1.])),
        ("annotations\\[0\\]\\[0\\].*run-length record", lambda: D.map_batch([img], [[dict(ann, segmentation={"size": [8, 9, 1], "counts": "X2"})]], t)),
    ]
    for pattern, call in bad_calls:
        with pytest.raises(ValueError, match=pattern):
            call()
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        D.preprocess_image([img.permute(2, 0, 1).cpu()], [1., 2., 3.], [1., 1., 1.])
    assert L._count[0] == before
    # a malformed run-length string is found on the device: list form raises after its one read, padded form drops the instance
    bad = dict(ann, segmentation={"size": [8, 9], "counts": "~~"})
    with pytest.raises(ValueError, match="run-length record 1"):
        D.map_batch([img], [[dict(ann, segmentation={"size": [8, 9], "counts": [10, 5, 57]}), bad]], t)
    pad = D.map_batch([img], [[dict(ann, segmentation={"size": [8, 9], "counts": [10, 5, 57]}), bad]], t, padded=True)
    assert pad[0]["keep"].tolist() == [True, False] and pad[0]["rle_status"].tolist()[0] == 0 and pad[0]["rle_status"].tolist()[1] != 0
    # the same with the malformed record among decoded masks: its word is there, the decoded masks' are 0; no records, no words
    mixed = D.map_batch([img], [[ann, bad, dict(ann, segmentation=torch.zeros((8, 9), dtype=torch.uint8))]], t, padded=True)
    st = mixed[0]["rle_status"].tolist()
    assert mixed[0]["keep"].tolist() == [True, False, False] and st[0] == 0 and st[1] != 0 and st[2] == 0
    assert D.map_batch([img], [[ann]], t, padded=True)[0]["rle_status"] is None
