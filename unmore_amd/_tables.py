"""What the detector-side modules (mask_loss, box_loss, copy_paste, labels) share on the host: reading Detectron2-style items, the
one-device check, the upload of a ctypes table of device pointers (_lib.RaggedSrc, CpPair, MlImage, BlImage -- the csrc files assert the
layouts these mirror), `workspace`, the one way from a umr_*_workspace byte count to a buffer (every module that calls such a function
uses it), and the bench tools' per-phase timing."""
import ctypes

import numpy as np
import torch

from . import _lib as L


def unwrap(v):
    return getattr(v, "tensor", v)                       # Detectron2's BitMasks / Boxes, or the tensor itself


def getter(item):
    """field name -> value or None, of a dict or of an object with Detectron2's Instances fields"""
    if isinstance(item, dict):
        return item.get
    return lambda name: getattr(item, name, None)


def as_u8(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def dtype_code(t):
    return L.BF16 if t.dtype == torch.bfloat16 else L.F32


def one_device(tensors, module, what, hint=""):
    """the one device of `tensors`: ValueError when they differ, RuntimeError when it is not the GPU"""
    devs = {t.device for t in tensors}
    if len(devs) > 1:
        raise ValueError(f"{module}: every tensor must be on the same device, got {sorted(str(d) for d in devs)}")
    dev = devs.pop()
    if dev.type != "cuda":
        raise RuntimeError(f"unmore_amd.{module}.{what} runs on the MI355X only (no CPU fallback); "
                           f"tests/{module}_common.py restates it on the host{hint}")
    return dev


def upload(table, n, dev, extras=()):
    """One host-to-device copy of the first n entries of a ctypes array, followed by the NumPy arrays `extras`: (uint8 buffer on `dev`,
    the byte offset of each extra in it).  The caller keeps what the table points into alive until its launches are enqueued."""
    parts = [np.frombuffer(table, dtype=np.uint8)[:ctypes.sizeof(table._type_) * n]]
    offs, end = [], parts[0].size
    for e in extras:
        parts.append(np.ascontiguousarray(e).reshape(-1).view(np.uint8))
        offs.append(end)
        end += parts[-1].size
    return torch.from_numpy(np.concatenate(parts)).to(dev), offs


def workspace(nbytes, dev):
    """The buffer for what a umr_*_workspace function returned: uint8, nbytes rounded up to a multiple of 16 and never empty, so its
    pointer is never NULL.  A negative count (the function refused its arguments) gives the 16 bytes too: the launch entry reports the
    error.  The entry point is still passed nbytes itself."""
    return torch.empty(max(16, (int(nbytes) + 15) // 16 * 16), dtype=torch.uint8, device=dev)


def timed(launch, parts, _phase_ms):
    """launch(phase mask) for all of `parts` = ((name, mask), ...) at once; with a dict (the bench tools) part by part between device
    events, the elapsed times added under the names -- that path ends in an event synchronisation, the product path makes the one call"""
    if _phase_ms is None:
        bits = 0
        for _, mask in parts:
            bits |= mask
        return launch(bits)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)]
    for i, (_, mask) in enumerate(parts):
        ev[i].record()
        launch(mask)
    ev[-1].record()
    ev[-1].synchronize()
    for i, (name, _) in enumerate(parts):
        _phase_ms[name] = _phase_ms.get(name, 0.0) + ev[i].elapsed_time(ev[i + 1])
