"""csrc/rle.hip on the GPU: the COCO run-length strings of umr_rle_encode (masks in memory) and umr_mask_paste_rle (the pasted union
masks of object scoring, never written) -- every comparison is byte equality of the string against unmore_amd.rle.encode_numpy of the
same mask (the CPU restatement pinned in test_rle_cpu.py) -- and Object_Scoring's `segmentation` records on the scoring fixture."""
import ctypes
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from discovery_stubs import FieldsFromCrop, ObjectFraction
from unmore_amd import rle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "scoring.npz"))
SCENES = {"a": (240, 320, 0, 4), "b": (200, 288, 5, 6)}


def _check(masks):
    """masks [K,H,W] u8 numpy: the device's records == the CPU's, string for string"""
    got = rle.encode(torch.from_numpy(masks).to(DEV))
    want = [rle.encode_numpy(m) for m in masks]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, masks.shape, len(g["counts"]), len(w["counts"]))
    return got


def _edge_cases(H, W, seed):
    """masks of very different run counts in one batch (the packing offsets differ for every one)"""
    rng = np.random.default_rng(seed)
    z = np.zeros((H, W), np.uint8)
    first, last, single = z.copy(), z.copy(), z.copy()
    first[0, 0] = 1
    last[H - 1, W - 1] = 1
    single[H // 2, W // 3] = 1
    alternating = (np.arange(H * W) % 2 == 0).astype(np.uint8).reshape((H, W), order="F")      # pixel 0 set: H*W + 1 runs
    stripes = np.repeat((np.arange(H) % 2).astype(np.uint8)[:, None], W, axis=1)
    noise = (rng.random((H, W)) < 0.5).astype(np.uint8)
    return np.stack([z, np.ones((H, W), np.uint8), first, last, single, alternating, stripes, noise])


@pytest.mark.parametrize("H,W", [(5, 7), (37, 53), (36, 52)])
def test_encode_edge_cases(H, W):
    masks = _edge_cases(H, W, seed=H)
    got = _check(masks)
    assert len(rle.string_to_counts(got[5]["counts"])) == H * W + 1
    assert got[0]["counts"] == rle.counts_to_string([H * W]) and got[0]["size"] == [H, W]


def test_encode_blobs_and_a_long_run():
    """150 x 210 (no multiple of the four-column load, of the strip or of the chunk): smoothed blobs, and a zero run longer than 2^14"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    blobs = (F.avg_pool2d(torch.randn(4, 1, 150, 210, generator=g), 15, 1, 7)[:, 0] > 0.02).to(torch.uint8).numpy()
    long_run = np.zeros((1, 150, 210), np.uint8)
    long_run[0, 140:, 205:] = 1
    long_run[0, 0, 0] = 1
    got = _check(np.concatenate([blobs, long_run]))
    assert rle.string_to_counts(got[4]["counts"]).max() > 2 ** 14


@pytest.mark.parametrize("shape", [(3, 1, 301), (3, 301, 1), (2, 3, 1500), (2, 4, 2052), (2, 1200, 150), (2, 1200, 152), (1, 64, 64)])
def test_encode_noise_across_strips_and_chunks(shape):
    """p = 0.5 noise puts run boundaries on every chunk, strip and wave edge: one row / one column (memory order), more columns than a
    strip holds (byte and dword loads), columns so high that a strip holds 64 of them, and K = 1"""
    rng = np.random.default_rng(shape[1] * 7 + shape[2])
    _check((rng.random(shape) < 0.5).astype(np.uint8))


def test_encode_the_pinned_five_character_group_bool_input_and_single_mask():
    m = np.zeros((1, 600000), np.uint8)
    m[0, 7:540000] = 1
    rec = rle.encode(torch.from_numpy(m).to(DEV))
    assert rec == {"size": [1, 600000], "counts": "7iZ_`0Pcj1"}
    b = torch.from_numpy(_edge_cases(9, 11, 1)).to(DEV)
    assert rle.encode(b.bool()) == rle.encode(b)
    assert rle.encode(b[7]) == rle.encode_numpy(b[7].cpu().numpy())
    assert rle.encode(b[:0]) == []


def _raw_encode(m, sizes=None, offsets=None, chars=None, cap=0, K=None, H=None, W=None):
    from unmore_amd import _lib as L
    from unmore_amd.ops import _p, _stream
    k, h, w = m.shape
    return L.lib().umr_rle_encode(_p(m), k if K is None else K, h if H is None else H, w if W is None else W, _p(sizes), _p(offsets), _p(chars), cap,
                                  _stream())


def test_two_passes_give_identical_bytes_and_respect_the_capacity():
    masks = torch.from_numpy(_edge_cases(37, 53, 2)).to(DEV)
    K = len(masks)
    outs = []
    for _ in range(2):
        sizes = torch.zeros((K, 2), dtype=torch.int64, device=DEV)
        assert _raw_encode(masks, sizes=sizes) == 0
        n = sizes.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(n[:, 1])]).astype(np.int64)
        chars = torch.full((int(off[-1]) + 64,), 255, dtype=torch.uint8, device=DEV)
        assert _raw_encode(masks, offsets=torch.from_numpy(off[:-1].copy()).to(DEV), chars=chars, cap=int(off[-1])) == 0
        outs.append((n, chars.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    n, chars = outs[0]
    assert n[:, 0].tolist() == [len(rle.mask_to_counts(m)) for m in masks.cpu().numpy()]
    assert (chars[-64:] == 255).all()
    # a capacity smaller than what the offsets ask for: nothing is stored at or beyond it
    total = int(n[:, 1].sum())
    short = torch.full((total,), 255, dtype=torch.uint8, device=DEV)
    off = np.concatenate([[0], np.cumsum(n[:, 1])]).astype(np.int64)
    assert _raw_encode(masks, offsets=torch.from_numpy(off[:-1].copy()).to(DEV), chars=short, cap=total - 100) == 0
    short = short.cpu().numpy()
    assert (short[total - 100:] == 255).all() and np.array_equal(short[:total - 100], chars[:total - 100])


def test_invalid_arguments_return_a_status_without_a_launch():
    from unmore_amd import _lib as L
    m = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    sizes = torch.full((2, 2), -7, dtype=torch.int64, device=DEV)
    chars = torch.full((16,), 255, dtype=torch.uint8, device=DEV)
    off = torch.zeros((2,), dtype=torch.int64, device=DEV)
    INVALID, UNSUPPORTED = -1, -2
    assert _raw_encode(m, sizes=sizes, K=0) == INVALID
    assert _raw_encode(m, sizes=sizes, H=0) == INVALID
    assert _raw_encode(m) == INVALID                                              # measure pass without sizes
    assert _raw_encode(m, chars=chars, cap=16) == INVALID                          # write pass without offsets
    assert _raw_encode(m, offsets=off, chars=chars, cap=0) == INVALID              # ... without a capacity
    assert _raw_encode(m, sizes=sizes, H=65536, W=32768) == INVALID                # H * W = 2^31
    assert _raw_encode(m, sizes=sizes, H=32768, W=2) == UNSUPPORTED                # four columns of that height do not fit the LDS
    assert b"32764" in L.lib().umr_last_error_string()
    from unmore_amd.ops import _p, _stream
    f = torch.zeros((1, 8, 8), device=DEV)
    c = torch.zeros((1, 2, 8, 8), device=DEV)
    bx = torch.tensor([[0, 0, 4, 4]], dtype=torch.int32, device=DEV)
    sel = torch.zeros((1,), dtype=torch.int64, device=DEV)
    lib = L.lib()
    assert lib.umr_mask_paste_rle(_p(f), _p(c), _p(bx), None, 1, 8, 16, 16, _p(sizes), None, None, 0, _stream()) == INVALID
    assert lib.umr_mask_paste_rle(_p(f), _p(c), _p(bx), _p(sel), 1, 8, 16, 16, None, None, None, 0, _stream()) == INVALID
    assert lib.umr_mask_paste_rle(_p(f), _p(c), _p(bx), _p(sel), 1, 300, 16, 16, _p(sizes), None, None, 0, _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (sizes.cpu() == -7).all() and (chars.cpu() == 255).all()


def test_pasted_rle_equals_the_rle_of_the_pasted_mask():
    """umr_mask_paste_rle against encode_numpy(umr_mask_paste(...)): the seven odd boxes and the seeded fields of
    test_object_scoring_gpu.py::test_pasted_mask_equals_torch_resize_of_a_random_mask, plus an empty box, boxes that end at the image's
    edges (on every side; as high as the image), boxes that reach beyond it, and a selection that permutes and repeats.  Both sides run
    the same paste_bit: any difference is a bug."""
    import torch.nn.functional as F
    from unmore_amd import _lib as L
    from unmore_amd.ops import _p, _stream
    g = torch.Generator().manual_seed(5)
    H, W, S = 150, 210, 128
    boxes = torch.tensor([[0, 0, W, H], [10, 20, 74, 84], [5, 7, 6, 140], [30, 40, 200, 43], [100, 3, 209, 149], [17, 90, 81, 122], [50, 50, 178, 178 - 28],
                          [40, 30, 40, 90],                                            # empty: x2 == x1
                          [150, 100, W, H], [0, 0, 33, 41], [120, 0, 180, H], [160, 0, W, H], [0, 60, W, 100],   # ending at the image's edges
                          [-9, -6, 70, 55], [170, 120, 240, 170]],                     # reaching beyond the image
                         dtype=torch.int32)
    N = len(boxes)
    sdf = (torch.randn(N, S, S, generator=g) * 0.7).contiguous()
    cen = (torch.randn(N, 2, S, S, generator=g) * 0.4).contiguous()
    sdf = F.avg_pool2d(sdf[:, None], 5, 1, 2)[:, 0].contiguous()
    cen = F.avg_pool2d(cen, 3, 1, 1).contiguous()
    # the lower rows / right columns of some crops set, so that masks touch the box's last row and column
    sdf[8:13, 100:, :] = 2.0
    sdf[8:13, :, 100:] = 2.0
    sel = torch.tensor([3, 0, 0, 14, 6, 2, 5, 1, 4, 7, 13, 8, 9, 12, 10, 11, 7, 0], dtype=torch.int64, device=DEV)
    K = len(sel)
    sd, cd, bd = sdf.to(DEV), cen.to(DEV), boxes.to(DEV)
    masks = torch.empty((K, H, W), dtype=torch.uint8, device=DEV)
    L.check(L.lib().umr_mask_paste(_p(sd), _p(cd), _p(bd), _p(sel), K, S, H, W, _p(masks), _stream()), "umr_mask_paste")
    got = rle.encode_pasted(sd, cd, bd, sel, H, W)
    m = masks.cpu().numpy()
    assert m[0].any() and not m[9].any()
    for k in range(K):
        assert got[k] == rle.encode_numpy(m[k]), (k, int(sel[k]), boxes[int(sel[k])].tolist())
    assert got[1] == got[2] == got[17]
    assert got == rle.encode(masks)


@pytest.mark.parametrize("tag", list(SCENES))
def test_object_scoring_segmentation(tag, tmp_path):
    from unmore_amd import synth
    from unmore_amd.object_scoring import Object_Scoring
    H, W, seed, nobj = SCENES[tag]
    image = torch.from_numpy(synth.reasoning_scene(H, W, seed, nobj)).to(DEV)
    raw = G[f"{tag}_raw_proposals"].tolist()
    osc = Object_Scoring(Namespace(), DEV, objectness_model=FieldsFromCrop(), binary_classifier_model=ObjectFraction())
    plain = osc.score_image(image, raw)
    assert sorted(plain) == sorted(["tight_bboxes", "masks", "score", "existence_score", "center_score", "boundary_score", "area_score", "keep"])
    out = osc.score_image(image, raw, segmentation=True)
    assert sorted(out) == sorted(list(plain) + ["segmentation"])
    assert torch.equal(out["masks"], plain["masks"]) and np.array_equal(out["score"], plain["score"])
    masks = out["masks"].cpu().numpy()
    K = len(masks)
    assert len(out["segmentation"]) == K >= 2
    tight = out["tight_bboxes"].cpu().numpy()
    for k in range(K):
        seg = out["segmentation"][k]
        assert seg["size"] == [H, W]
        assert np.array_equal(rle.decode_numpy(seg), masks[k])
        assert rle.area(seg) == int(masks[k].sum())
        x1, y1, x2, y2 = tight[k].tolist()
        assert rle.to_bbox(seg) == [x1, y1, x2 - x1, y2 - y1]
    lean = osc.score_image(image, raw, segmentation=True, masks=False)
    assert lean["masks"] is None and lean["segmentation"] == out["segmentation"]
    assert np.array_equal(lean["score"], out["score"]) and torch.equal(lean["tight_bboxes"], out["tight_bboxes"])
    # the stage's file
    path = tmp_path / "object_discovery_with_scores.json"
    records = osc.main_object_scoring([(17, image), (18, image)], {"17": raw}, segmentation=True, out_path=path)
    back = json.loads(path.read_text())
    assert len(back) == len(records) == K
    keys = ["image_id", "category_id", "score", "bbox", "segmentation", "existence_score", "center_score", "boundary_score", "area_score"]
    for k, r in enumerate(back):
        assert list(r) == keys and r["image_id"] == 17 and r["segmentation"] == out["segmentation"][k]
        assert r["score"] == float(out["score"][k]) and type(r["area_score"]) is float and len(r["bbox"]) == 4
    assert osc.main_object_scoring([(17, image)], {"17": raw})[0].keys() == set(keys) - {"segmentation"}
