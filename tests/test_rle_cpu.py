"""unmore_amd.rle on the CPU: the numpy restatement of pycocotools' run-length string (the format the device kernels of csrc/rle.hip
are compared against in test_rle_gpu.py), pinned on hand-checked strings, round trips on random masks and on the reference-made final
masks of tests/golden/scoring.npz; Object_Scoring's records with and without `segmentation`, and the JSON writer."""
import json
import os

import numpy as np
import pytest

from unmore_amd import rle

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "scoring.npz"))


def _m(H, W, *ones):
    m = np.zeros((H, W), np.uint8)
    for ys, xs in ones:
        m[ys, xs] = 1
    return m


_CHECKER = (np.add.outer(np.arange(3), np.arange(3)) % 2 == 0).astype(np.uint8)
PINNED = [
    ("zeros", _m(3, 4), [12], "<"),
    ("ones", np.ones((3, 4), np.uint8), [0, 12], "0<"),
    ("one pixel", _m(3, 4, (1, 2)), [7, 1, 4], "714"),
    ("rectangle", _m(4, 5, (slice(1, 3), slice(1, 4))), [5, 2, 2, 2, 2, 2, 5], "5220003"),
    ("checkerboard", _CHECKER, [0, 1, 1, 1, 1, 1, 1, 1, 1, 1], "0110000000"),
    ("negative delta", _m(1, 40, (0, slice(0, 20)), (0, slice(21, 23))), [0, 20, 1, 2, 17], "0d01^O`0"),
    ("block 40x40", _m(40, 40, (slice(5, 35), slice(8, 20))), None, "U:n0:000000000000000000000kh0"),
    ("five characters", _m(1, 600000, (0, slice(7, 540000))), [7, 539993, 60000], "7iZ_`0Pcj1"),
]


@pytest.mark.parametrize("name,mask,counts,string", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_strings(name, mask, counts, string):
    got = rle.mask_to_counts(mask)
    if counts is None:
        assert len(got) == 25
    else:
        assert got.tolist() == counts
    rec = rle.encode_numpy(mask)
    assert rec == {"size": list(mask.shape), "counts": string}
    assert rle.counts_to_string(got) == string
    assert rle.string_to_counts(string).tolist() == got.tolist()
    assert np.array_equal(rle.decode_numpy(rec), mask)
    assert rle.area(rec) == int(mask.sum())


def _tight(mask):
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def test_round_trip_of_random_masks():
    rng = np.random.default_rng(11)
    for _ in range(200):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        m = (rng.random((H, W)) < rng.random()).astype(np.uint8)
        rec = rle.encode_numpy(m)
        assert rec["size"] == [H, W] and rec["counts"].isascii()
        assert np.array_equal(rle.decode_numpy(rec), m)
        assert rle.area(rec) == int(m.sum())
        assert rle.to_bbox(rec) == _tight(m)


@pytest.mark.parametrize("tag,characters", [("a", 1527), ("b", 766)])
def test_reference_made_final_masks(tag, characters):
    shape = tuple(G[f"{tag}_final_masks_shape"])
    masks = np.unpackbits(G[f"{tag}_final_masks_packed"])[:int(np.prod(shape))].reshape(shape)
    empty, total = 0, 0
    for m in masks:
        rec = rle.encode_numpy(m)
        total += len(rec["counts"])
        assert np.array_equal(rle.decode_numpy(rec), m)
        assert rle.to_bbox(rec) == _tight(m) and rle.area(rec) == int(m.sum())
        if not m.any():
            empty += 1
            assert rle.string_to_counts(rec["counts"]).tolist() == [shape[1] * shape[2]]
    assert empty == 1                       # the last survivor of either scene is an empty mask
    assert total == characters              # against masks.size = 460 800 / 115 200 bytes


def _scored(with_segmentation):
    import torch
    s = {"tight_bboxes": torch.tensor([[2.0, 3.0, 10.0, 9.0], [0.0, 0.0, 0.0, 0.0]]), "masks": None,
         "score": np.array([0.25, 0.0], np.float64), "existence_score": np.array([0.5, 0.1], np.float32),
         "center_score": np.array([1.5, 0.2], np.float32), "boundary_score": np.array([0.75, 0.3], np.float32),
         "area_score": np.array([1.0, 0.0], np.float64), "keep": torch.tensor([1, 0])}
    if with_segmentation:
        s["segmentation"] = [rle.encode_numpy(_m(12, 16, (slice(3, 9), slice(2, 10)))), rle.encode_numpy(_m(12, 16))]
    return s


REFERENCE_KEYS = ["image_id", "category_id", "score", "bbox", "segmentation", "existence_score", "center_score", "boundary_score", "area_score"]


def test_annotations_with_and_without_segmentation():
    from unmore_amd.object_scoring import Object_Scoring
    osc = Object_Scoring.__new__(Object_Scoring)          # annotations() uses no state
    plain = osc.annotations(7, _scored(False))
    assert [list(r) for r in plain] == [[k for k in REFERENCE_KEYS if k != "segmentation"]] * 2
    full = osc.annotations(7, _scored(True))
    assert [list(r) for r in full] == [REFERENCE_KEYS] * 2          # the reference's key order (object_scoring.py:257-267)
    assert full[0]["segmentation"] == {"size": [12, 16], "counts": rle.encode_numpy(_m(12, 16, (slice(3, 9), slice(2, 10))))["counts"]}
    assert full[0]["bbox"] == [2.0, 3.0, 8.0, 6.0] and rle.to_bbox(full[0]["segmentation"]) == [2.0, 3.0, 8.0, 6.0]
    assert rle.to_bbox(full[1]["segmentation"]) == [0.0] * 4 and full[1]["segmentation"]["counts"] == rle.counts_to_string([12 * 16])
    for a, b in zip(plain, full):
        assert {k: v for k, v in b.items() if k != "segmentation"} == a
    assert osc.annotations(7, None) == []


def test_json_writer_converts_numpy_values(tmp_path):
    from unmore_amd.object_scoring import Object_Scoring, write_annotations
    osc = Object_Scoring.__new__(Object_Scoring)
    records = osc.annotations(np.int64(7), _scored(True))
    assert isinstance(records[0]["score"], np.floating) and isinstance(records[0]["existence_score"], np.float32)
    records[0]["extra"] = {"array": np.arange(3, dtype=np.int32), "flag": np.bool_(True), "n": np.uint8(5)}
    path = tmp_path / "object_discovery_with_scores.json"
    write_annotations(records, path)
    text = path.read_text()
    assert text.startswith("[\n  {\n    \"image_id\": 7,")              # indent=2, as the reference writes it
    back = json.loads(text)
    assert len(back) == 2 and list(back[0])[:9] == REFERENCE_KEYS
    for k in ("score", "existence_score", "center_score", "boundary_score", "area_score"):
        assert type(back[0][k]) is float
    assert back[0]["existence_score"] == 0.5 and back[0]["center_score"] == 1.5 and back[0]["bbox"] == [2.0, 3.0, 8.0, 6.0]
    assert back[0]["extra"] == {"array": [0, 1, 2], "flag": True, "n": 5}
    assert np.array_equal(rle.decode_numpy(back[0]["segmentation"]), _m(12, 16, (slice(3, 9), slice(2, 10))))
    with pytest.raises(TypeError):
        write_annotations([{"x": object()}], tmp_path / "bad.json")
