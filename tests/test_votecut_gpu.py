"""csrc/rle_decode.hip on the GPU: run-length strings parsed and painted on the device (rle.decode), the largest 4-connected component
by run labelling (rle.largest_component), and VoteCutAnnotations.masks feeding the two item synthesisers.  Every comparison is byte
equality against the host: rle.decode_numpy, numpy's OR, and votecut_common.largest_numpy (pinned by hand in test_votecut_cpu.py)."""
import numpy as np
import pytest
import torch

from unmore_amd import VoteCutAnnotations, rle
from votecut_common import (BIG, DECODE_PATTERNS, LARGEST_PATTERNS, SIZES, blob, counts_to_mask, largest_numpy, pattern, zero_run_record)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PINNED = {"size": [1, 600000], "counts": "7iZ_`0Pcj1"}          # a five-character group


def _same(got, want, what):
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape, what
    assert np.array_equal(got.cpu().numpy(), want), what


def test_decode_equals_the_host_decoder():
    recs, names = [], []
    for (H, W) in SIZES:
        for name in DECODE_PATTERNS:
            recs.append(rle.encode_numpy(pattern(name, H, W)))
            names.append((name, H, W))
    recs += [PINNED, zero_run_record(9, 5), zero_run_record(33, 65)]
    names += ["pinned", "zero runs 9x5", "zero runs 33x65"]
    recs.append({"size": [5, 7], "counts": rle.encode_numpy(pattern("noise", 5, 7))["counts"].encode("ascii")})    # bytes
    names.append("bytes")
    got = rle.decode(recs, device=DEV)
    assert len(got) == len(recs)
    for g, r, n in zip(got, recs, names):
        _same(g, rle.decode_numpy(rle.as_record(r)) * 255, n)
    assert int(got[names.index("pinned")].sum()) == 539993 * 255
    z = zero_run_record(9, 5)
    _same(got[names.index("zero runs 9x5")], counts_to_mask(z["counts"], 9, 5) * 255, "zero runs against the count list itself")
    assert len({g.data_ptr() for g in got}) == len(got)                  # one packed buffer, every offset differs


def test_union_of_groups():
    rng = np.random.default_rng(5)
    a = [(rng.random((33, 65)) < 0.2).astype(np.uint8) for _ in range(3)]
    b = [pattern("noise", 5, 7)]
    c = [blob(150, 210, s) for s in range(3)]
    records = [rle.encode_numpy(m) for m in a + b + c]
    groups = [(3, (33, 65)), (0, (9, 1)), (1, (5, 7)), (0, (64, 64)), (3, (150, 210))]
    got = rle.decode(records, groups=groups, device=DEV)
    want = [a[0] | a[1] | a[2], np.zeros((9, 1), np.uint8), b[0], np.zeros((64, 64), np.uint8), c[0] | c[1] | c[2]]
    assert len(got) == 5
    for g, w in zip(got, want):
        _same(g, w * 255, "union")
    assert 0 < int(want[0].sum()) < 33 * 65


def _check_largest(recs, names):
    got, info = rle.largest_component(recs, device=DEV)
    info = info.cpu().numpy()
    assert info.shape == (len(recs), 2) and info.dtype == np.int32
    for k, (g, r, n) in enumerate(zip(got, recs, names)):
        want, want_info = largest_numpy(rle.decode_numpy(rle.as_record(r)))
        print(n, "components, area: device", tuple(info[k]), "host", want_info)
        assert tuple(int(v) for v in info[k]) == want_info, n
        _same(g, want, n)
    return got, info


def test_largest_component_small_sizes():
    recs, names = [], []
    for (H, W) in SIZES:
        for name in LARGEST_PATTERNS:
            recs.append(rle.encode_numpy(pattern(name, H, W)))
            names.append((name, H, W))
    for (H, W) in [(9, 5), (33, 65), (150, 210)]:
        recs.append(zero_run_record(H, W))
        names.append(("zero-run touch", H, W))
    got, info = _check_largest(recs, names)
    by = {n: k for k, n in enumerate(names)}
    k = by[("tie", 33, 65)]                                              # the top-right block wins; column-major order would pick the other
    assert tuple(info[k]) == (2, 4) and int(got[k][0, 64]) == 255 and int(got[k][32, 0]) == 0
    assert tuple(info[by[("wrap", 33, 65)]]) == (2, 1)                   # one run of length 2, two components
    assert tuple(info[by[("diagonal", 64, 64)]]) == (64, 1)
    assert tuple(info[by[("serpentine", 150, 210)]])[0] == 1 and tuple(info[by[("comb", 150, 210)]])[0] == 1
    assert tuple(info[by[("zero-run touch", 33, 65)]]) == (2, 6)         # 2 + 4 pixels that touch inside a column


def test_largest_component_375x500():
    H, W = BIG
    names = [(n, H, W) for n in LARGEST_PATTERNS] + [("blob", H, W)]
    recs = [rle.encode_numpy(pattern(n, H, W)) for n in LARGEST_PATTERNS] + [rle.encode_numpy(blob(H, W, 1))]
    got, info = _check_largest(recs, names)
    assert tuple(info[LARGEST_PATTERNS.index("checkerboard")]) == (93750, 1)          # parents beyond LDS
    assert int(got[LARGEST_PATTERNS.index("checkerboard")].sum()) == 255 and int(got[LARGEST_PATTERNS.index("checkerboard")][0, 0]) == 255
    assert tuple(info[LARGEST_PATTERNS.index("serpentine_t")])[0] == 1


def _malformed():
    good = rle.encode_numpy(pattern("noise", 33, 65))["counts"]
    return {
        "truncated": good[:len(good) // 2],
        "stops inside a number": rle.counts_to_string([100, 33 * 65 - 100])[:-1],
        "sum too large": good + "5",
        "negative count": rle.counts_to_string([-3, 33 * 65 + 3]),
        "character below '0'": good[:7] + "/" + good[8:],
        "character above 'o'": good[:7] + "~" + good[8:],
        "empty string": "",
    }


@pytest.mark.parametrize("case", list(_malformed()))
@pytest.mark.parametrize("fn", ["decode", "largest_component"])
def test_malformed_strings_are_rejected(fn, case):
    """rejected by the validation pass: status, an all-zero mask, the other records of the call untouched"""
    first, last = pattern("noise", 5, 7), blob(150, 210, 2)
    recs = [rle.encode_numpy(first), {"size": [33, 65], "counts": _malformed()[case]}, rle.encode_numpy(last)]
    runs = []
    for _ in range(2):
        with pytest.raises(ValueError, match="record 1 ") as e:
            getattr(rle, fn)(recs, device=DEV)
        assert list(np.flatnonzero(e.value.status)) == [1]
        runs.append([m.cpu().numpy() for m in e.value.masks])
    ref = (lambda m: largest_numpy(m)[0]) if fn == "largest_component" else (lambda m: m * 255)
    assert np.array_equal(runs[0][0], ref(first)) and np.array_equal(runs[0][2], ref(last))
    assert runs[0][1].shape == (33, 65) and not runs[0][1].any()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def _annotations():
    sizes = {11: (150, 210), 4: (120, 96), 9: (64, 64)}
    images, anns, host = [], [], {}
    for i, (H, W) in sizes.items():
        images.append({"id": i, "file_name": f"n{i:02d}/x{i}.JPEG", "height": H, "width": W})
        ms = [blob(H, W, 10 * i + j) for j in range(3)]
        weights = [0.2, 0.7, 0.7]
        for j, (m, wt) in enumerate(zip(ms, weights)):
            anns.append({"id": 100 * i + j, "image_id": i, "weight": wt, "segmentation": rle.encode_numpy(m)})
        host[i] = (largest_numpy(ms[1])[0], ((ms[0] | ms[1] | ms[2]) * 255).astype(np.uint8))
    images.append({"id": 20, "file_name": "n20/none.JPEG", "height": 8, "width": 8})
    anns = anns[::3] + anns[1::3] + anns[2::3]                            # annotations of one image are not adjacent in the file
    return {"images": images, "annotations": anns}, sizes, host


def test_annotations_to_training_items():
    from unmore_amd import synthesize_classifier_items
    from unmore_amd.labels import synthesize_training_items
    d, sizes, host = _annotations()
    ann = VoteCutAnnotations(d)
    ids = ann.image_ids
    assert ids == [4, 9, 11]
    top1, full = ann.masks(ids, device=DEV)
    for i, t, f in zip(ids, top1, full):
        _same(t, host[i][0], ("top-1", i))
        _same(f, host[i][1], ("full", i))
    rng = np.random.default_rng(2)
    images = [torch.from_numpy(rng.random((3,) + sizes[i], dtype=np.float32)).to(DEV) for i in ids]
    h_top1 = [torch.from_numpy(host[i][0]).to(DEV) for i in ids]
    h_full = [torch.from_numpy(host[i][1]).to(DEV) for i in ids]
    coins = [True, False, True]
    params = [(10, 8, 60, 50), (5, 6, 40, 44), (20, 30, 100, 120)]
    got = synthesize_classifier_items(images, top1, full, 64, coins=coins, params=params)
    want = synthesize_classifier_items(images, h_top1, h_full, 64, coins=coins, params=params)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for key in ("branch", "boxes", "mask_sum"):
        assert torch.equal(got[2][key], want[2][key]), key
    assert float(got[1].sum()) > 0
    p400 = [(40, 30, 300, 280), (0, 0, 400, 400), (100, 120, 200, 160)]
    gi, gl, _ = synthesize_training_items(images, top1, 64, params=p400)
    wi, wl, _ = synthesize_training_items(images, h_top1, 64, params=p400)
    assert torch.equal(gi, wi)
    for key in wl:
        assert torch.equal(gl[key], wl[key]), key
    assert float(gl["instance_mask"].sum()) > 0


def test_mode_1_group_table_seen_on_the_device_only():
    """K == G passes the host check of the C entry point; a group_start that still gives one group two records and another none is
    reported through the records' status (8 = table), with all-zero masks"""
    import ctypes
    from unmore_amd import _lib as L
    recs = [rle.encode_numpy(pattern("full", 5, 7))["counts"].encode("ascii")] * 2
    K = G = 2
    chars = torch.tensor(list(b"".join(recs)), dtype=torch.uint8, device=DEV)
    n = len(recs[0])
    char_offsets = torch.tensor([0, n, 2 * n], dtype=torch.int64, device=DEV)
    out_desc = torch.tensor([[5, 7, 0], [5, 7, 48]], dtype=torch.int64, device=DEV)
    seg = n // 2 + 1 + 7
    seg_offsets = torch.tensor([0, seg, 2 * seg], dtype=torch.int64, device=DEV)
    out = torch.full((96,), 7, dtype=torch.uint8, device=DEV)
    info = torch.full((G, 2), -1, dtype=torch.int32, device=DEV)
    nbytes = L.lib().umr_rle_decode_workspace(K, 2 * n, 2 * seg, 1)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    res = {}
    for name, gs in (("bad", [0, 2, 2]), ("good", [0, 1, 2])):
        group_start = torch.tensor(gs, dtype=torch.int32, device=DEV)
        status = torch.full((K,), -1, dtype=torch.int32, device=DEV)
        out.fill_(7)
        L.check(L.lib().umr_rle_decode(p(chars), p(char_offsets), K, 2 * n, p(out_desc), p(group_start), p(seg_offsets), G, 35, 2 * seg, p(out), 96,
                                       255, 1, p(status), p(info), p(ws), nbytes, None), "umr_rle_decode")
        torch.cuda.synchronize()
        res[name] = (status.cpu().tolist(), info.cpu().tolist(), out.cpu().numpy().copy())
    assert res["bad"][0] == [8, 8] and res["bad"][1] == [[0, 0], [0, 0]]
    assert not res["bad"][2][:35].any() and not res["bad"][2][48:83].any() and (res["bad"][2][35:48] == 7).all()
    assert res["good"][0] == [0, 0] and res["good"][1] == [[1, 35], [1, 35]]
    assert (res["good"][2][:35] == 255).all() and (res["good"][2][48:83] == 255).all() and (res["good"][2][35:48] == 7).all()
