"""unmore_amd.votecut / the decode direction of unmore_amd.rle without a GPU: the annotation index, the argument errors that are raised
before any launch, the record forms, and the host checker the GPU tests compare against (pinned on masks worked out by hand)."""
import ctypes

import numpy as np
import pytest

from unmore_amd import VoteCutAnnotations, rle
from votecut_common import ZERO_RUN_COUNTS, counts_to_mask, largest_numpy, pattern, zero_run_record


def _rec(H, W):
    return rle.encode_numpy(np.zeros((H, W), np.uint8))


ANNOTATIONS = {
    "images": [{"id": 7, "file_name": "n01/a.JPEG", "height": 4, "width": 5}, {"id": 3, "file_name": "n02/b.JPEG", "height": 2, "width": 2},
               {"id": 5, "file_name": "n03/c.JPEG", "height": 3, "width": 3}, {"id": 1, "file_name": "n04/d.JPEG", "height": 6, "width": 2}],
    "annotations": [{"id": 10, "image_id": 7, "weight": 0.5, "segmentation": {"size": [4, 5], "counts": "a"}},
                    {"id": 11, "image_id": 3, "weight": 0.1, "segmentation": {"size": [2, 2], "counts": "b"}},
                    {"id": 12, "image_id": 7, "weight": 0.9, "segmentation": {"size": [4, 5], "counts": "c"}},
                    {"id": 13, "image_id": 1, "weight": 0.3, "segmentation": {"size": [6, 2], "counts": "d"}},
                    {"id": 14, "image_id": 7, "weight": 0.9, "segmentation": {"size": [4, 5], "counts": "e"}},
                    {"id": 15, "image_id": 1, "weight": 0.3, "segmentation": {"size": [6, 2], "counts": "f"}}],
}


def test_annotation_index():
    a = VoteCutAnnotations(ANNOTATIONS)
    assert a.image_ids == [1, 3, 7] and len(a) == 3                     # sorted; image 5 has no annotation and is left out
    assert a.file_name(7) == "n01/a.JPEG" and a.file_name(5) == "n03/c.JPEG"
    assert [r["counts"] for r in a.records(7)] == ["a", "c", "e"]       # file order
    assert [r["counts"] for r in a.records(1)] == ["d", "f"]
    assert a.top1(7)["id"] == 12                                        # two equal weights: the earlier one, as np.argmax
    assert a.top1(1)["id"] == 13
    assert a.top1(3)["id"] == 11
    with pytest.raises(KeyError):
        a.top1(5)


def test_annotation_file(tmp_path):
    import json
    p = tmp_path / "ann.json"
    p.write_text(json.dumps(ANNOTATIONS))
    a = VoteCutAnnotations(str(p))
    assert a.image_ids == [1, 3, 7] and a.top1(7)["id"] == 12


def test_argument_errors_are_raised_before_any_launch():
    """device='cpu' would raise RuntimeError at the launch: every one of these is a ValueError, so none got that far"""
    polygon = [[1.0, 1.0, 4.0, 1.0, 4.0, 4.0]]
    for fn in (rle.decode, rle.largest_component):
        with pytest.raises(ValueError, match="record 1.*polygon"):
            fn([_rec(3, 3), polygon], device="cpu")
        with pytest.raises(ValueError, match="record 0"):
            fn([{"size": [0, 4], "counts": "0"}], device="cpu")
        with pytest.raises(ValueError, match="record 0"):
            fn([{"size": [-2, 4], "counts": "0"}], device="cpu")
        with pytest.raises(ValueError, match="record 0"):
            fn([{"size": [1 << 16, 1 << 15], "counts": "0"}], device="cpu")
    with pytest.raises(ValueError, match="record 1 has size.*group 0"):
        rle.decode([_rec(3, 4), _rec(4, 3)], groups=[(2, (3, 4))], device="cpu")
    with pytest.raises(ValueError, match="group 1"):
        rle.decode([_rec(3, 4)], groups=[(1, (3, 4)), (0, (0, 4))], device="cpu")
    with pytest.raises(ValueError):
        rle.decode([_rec(3, 4), _rec(3, 4)], groups=[(1, (3, 4))], device="cpu")        # a record left over
    with pytest.raises(ValueError):
        rle.decode([_rec(3, 4)], groups=[(2, (3, 4))], device="cpu")                    # a record too few
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rle.decode([_rec(3, 4)], device="cpu")
    assert rle.decode([], device="cpu") == []


def test_mode_1_takes_one_record_per_group():
    from unmore_amd import _lib
    with pytest.raises(ValueError, match="group 0 holds 2 records"):
        rle._prepare([_rec(3, 4), _rec(3, 4)], [(2, (3, 4))], 1, "largest_component")
    lib = _lib.lib()
    # host buffers of the sizes the arguments name: the argument checks answer before any launch, and nothing here points nowhere
    K, G, nchars, nseg = 2, 1, 10, 20
    chars = (ctypes.c_uint8 * nchars)(*([ord("0")] * nchars))
    char_offsets = (ctypes.c_int64 * (K + 1))(0, 5, 10)
    out_desc = (ctypes.c_int64 * 3)(3, 4, 0)
    group_start = (ctypes.c_int32 * (G + 1))(0, 2)
    seg_offsets = (ctypes.c_int64 * (G + 1))(0, nseg)
    out = (ctypes.c_uint8 * 16)()
    status = (ctypes.c_int32 * K)()
    info = (ctypes.c_int32 * (2 * G))()
    nbytes = lib.umr_rle_decode_workspace(K, nchars, nseg, 1)
    ws = (ctypes.c_uint8 * nbytes)()

    def call(K, mode, ws_bytes):
        return lib.umr_rle_decode(chars, char_offsets, K, nchars, out_desc, group_start, seg_offsets, G, 12, nseg, out, 16, 255, mode, status, info,
                                  ws, ws_bytes, None)
    assert call(2, 1, nbytes) == -1                                     # UMR_ERR_INVALID: K != G in mode 1
    assert b"mode 1" in lib.umr_last_error_string()
    assert call(1, 2, nbytes) == -1
    assert call(1, 0, 8) == -1
    assert b"workspace" in lib.umr_last_error_string()
    assert lib.umr_rle_decode_workspace(1, 10, 20, 1) > lib.umr_rle_decode_workspace(1, 10, 20, 0) >= 11 * 12 + 4
    assert lib.umr_rle_decode_workspace(1, -1, 0, 0) == -1


def test_uncompressed_counts_convert_to_the_same_record():
    rng = np.random.default_rng(3)
    m = (rng.random((13, 9)) < 0.4).astype(np.uint8)
    want = rle.encode_numpy(m)
    counts = [int(c) for c in rle.mask_to_counts(m)]
    assert rle.as_record({"size": [13, 9], "counts": counts}) == want
    assert rle.as_record({"size": [13, 9], "counts": want["counts"].encode("ascii")}) == want
    z = rle.as_record(zero_run_record(9, 5))
    assert list(rle.string_to_counts(z["counts"]))[:len(ZERO_RUN_COUNTS) - 1] == ZERO_RUN_COUNTS[:-1]
    assert (rle.decode_numpy(z) == counts_to_mask(zero_run_record(9, 5)["counts"], 9, 5)).all()
    assert rle.string_to_counts("7iZ_`0Pcj1").tolist() == [7, 539993, 60000]             # the five-character group


def test_the_checker_on_masks_worked_out_by_hand():
    a = np.array([[1, 1, 0, 0, 1],
                  [0, 1, 0, 1, 1],
                  [0, 0, 0, 0, 1],
                  [1, 0, 0, 0, 1]], np.uint8)
    got, info = largest_numpy(a)
    want = np.array([[0, 0, 0, 0, 1],
                     [0, 0, 0, 1, 1],
                     [0, 0, 0, 0, 1],
                     [0, 0, 0, 0, 1]], np.uint8) * 255
    assert (got == want).all() and info == (3, 5) and got.dtype == np.uint8
    # 4-connected: a diagonal is three components of area 1, the first in raster order is kept
    got, info = largest_numpy(np.eye(3, dtype=np.uint8))
    assert (got == np.array([[255, 0, 0], [0, 0, 0], [0, 0, 0]])).all() and info == (3, 1)
    # the tie: equal areas, the block whose first raster pixel comes first (top right) wins, not the first in column-major order
    t = pattern("tie", 6, 7)
    assert t.sum() == 8 and t[0, 5] and t[5, 0]
    got, info = largest_numpy(t)
    want = np.zeros((6, 7), np.uint8)
    want[:2, 5:] = 255
    assert (got == want).all() and info == (2, 4)
    got, info = largest_numpy(np.zeros((2, 3), np.uint8))
    assert not got.any() and info == (0, 0)
