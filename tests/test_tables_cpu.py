"""unmore_amd._tables without a GPU: the layouts of the ctypes mirrors of the device tables (the csrc files assert the same numbers on the C
structs), the upload of a table with its extras, the workspace buffer, the one-device check and the untimed path of `timed`."""
import ctypes

import numpy as np
import pytest
import torch

from unmore_amd import _lib as L
from unmore_amd import _tables as T


@pytest.mark.parametrize("mirror,size,last,offset", [(L.RaggedSrc, 24, "W", 20), (L.CpPair, 152, "reserved", 148),
                                                     (L.MlImage, 48, "index64", 44), (L.BlImage, 56, "width", 52),
                                                     (L.DpImage, 48, "width", 44)])
def test_mirrors_keep_the_layout_the_kernels_assert(mirror, size, last, offset):
    assert ctypes.sizeof(mirror) == size
    assert mirror._fields_[-1][0] == last and getattr(mirror, last).offset == offset


def _filled(n):
    tab = (L.MlImage * n)()
    for k in range(n):
        tab[k].masks, tab[k].boxes, tab[k].index = 0x1000 + k, 0x2000 + k, None
        tab[k].H, tab[k].W, tab[k].G, tab[k].first, tab[k].R, tab[k].index64 = 3 + k, 5 + k, 7, 11 * k, 13, k & 1
    return tab


def test_upload_copies_the_first_entries_then_the_extras():
    tab = _filled(3)
    extras = [np.arange(5, dtype=np.int32), np.array([[1.5, -2.0]], dtype=np.float32)]
    buf, offs = T.upload(tab, 2, torch.device("cpu"), extras)
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    raw, n = buf.numpy().tobytes(), 2 * ctypes.sizeof(L.MlImage)
    assert raw[:n] == bytes(tab)[:n]
    assert offs == [n, n + 20] and len(raw) == n + 28
    assert raw[offs[0]:offs[1]] == extras[0].tobytes() and raw[offs[1]:] == extras[1].tobytes()
    tab[0].H = 99                                          # the buffer is a copy, not a view of the table
    assert buf.numpy().tobytes() == raw
    plain, none = T.upload(tab, 3, torch.device("cpu"))
    assert none == [] and plain.numpy().tobytes() == bytes(tab)


def test_upload_of_no_entries_is_an_empty_table():
    buf, offs = T.upload((L.BlImage * 1)(), 0, torch.device("cpu"))
    assert buf.dtype == torch.uint8 and buf.numel() == 0 and offs == []


def test_workspace_rounds_up_to_16_bytes_and_is_never_empty():
    for nbytes, size in ((0, 16), (1, 16), (16, 16), (17, 32), (-1, 16)):    # -1: what a *_workspace function returns for bad arguments
        ws = T.workspace(nbytes, torch.device("cpu"))
        assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() == size and ws.device.type == "cpu", nbytes


def test_one_device():
    cpu = torch.zeros(2)
    with pytest.raises(ValueError, match=r"^box_loss: every tensor must be on the same device, got \['cpu', 'meta'\]$"):
        T.one_device([cpu, torch.zeros(2, device="meta"), cpu], "box_loss", "get_deltas")
    with pytest.raises(RuntimeError, match=r"^unmore_amd\.mask_loss\.mask_targets runs on the MI355X only \(no CPU fallback\); "
                                           r"tests/mask_loss_common\.py restates it on the host \(see there\)$"):
        T.one_device([cpu, cpu], "mask_loss", "mask_targets", " (see there)")
    with pytest.raises(RuntimeError, match=r"tests/box_loss_common\.py restates it on the host$"):
        T.one_device([cpu], "box_loss", "get_deltas")


def test_timed_without_a_dict_is_one_launch_of_every_part():
    calls = []
    T.timed(calls.append, (("resize_paste", 1), ("overlap", 2), ("compose", 4)), None)
    assert calls == [7]
    calls.clear()
    T.timed(calls.append, (("match", 1),), None)
    assert calls == [1]
