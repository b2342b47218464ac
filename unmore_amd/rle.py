"""COCO run-length encoding of binary masks: the `segmentation` of the records object scoring writes (object_scoring.py:166-170,257-272).

The format is pycocotools' (maskApi.c).  For a mask [H,W] of 0/1 the pixels are taken in column-major order, j = x*H + y; `counts` are the
lengths of the alternating runs, starting with a run of zeros (0 when pixel 0 is set; an all-zero mask is the single count H*W).  The
string writes, for run i, x = counts[i] - (counts[i-2] if i > 2 else 0) as a signed number in 5-bit groups, low group first: after
c = x & 0x1f and x >>= 5 (arithmetic) another group follows iff (x != -1 if c & 0x10 else x != 0); a group that is followed by another
has 0x20 set; every group is the character chr(c + 48).  A record is {"size": [H, W], "counts": str}.

`encode` / `encode_pasted` run on the device (csrc/rle.hip): a measure pass, one small read of the sizes, a write pass into a packed
buffer, one read of the characters -- nothing image-sized crosses to the host.  The *_numpy functions restate the format on the CPU:
what the tests compare the kernels against and what a host without a GPU reads the file back with."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------- the format on the CPU
def mask_to_counts(mask):
    """[H,W] 0/1 -> the run lengths (int64 array), column-major, starting with zeros"""
    m = np.asarray(mask)
    assert m.ndim == 2, "a mask is [H, W]"
    flat = (m != 0).reshape(-1, order="F") if m.size else np.zeros(0, bool)
    change = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)) != 0)   # position j: pixel j differs from pixel j-1
    bounds = np.concatenate([[0], change, [flat.size]]).astype(np.int64)
    return np.diff(bounds)


def counts_to_string(counts):
    out = bytearray()
    cs = [int(c) for c in counts]
    for i, c in enumerate(cs):
        x = c - (cs[i - 2] if i > 2 else 0)
        more = True
        while more:
            g = x & 0x1f
            x >>= 5
            more = (x != -1) if (g & 0x10) else (x != 0)
            if more:
                g |= 0x20
            out.append(g + 48)
    return out.decode("ascii")


def string_to_counts(s):
    if isinstance(s, str):
        s = s.encode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            g = s[p] - 48
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and (g & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.asarray(counts, dtype=np.int64)


def encode_numpy(mask):
    m = np.asarray(mask)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts_to_string(mask_to_counts(m))}


def decode_numpy(rle):
    """record -> [H,W] u8"""
    H, W = rle["size"]
    counts = string_to_counts(rle["counts"])
    assert int(counts.sum()) == H * W and (counts >= 0).all(), "counts do not cover the mask"
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return flat.reshape((H, W), order="F")


def area(rle):
    """number of set pixels (pycocotools' `area`)"""
    return int(string_to_counts(rle["counts"])[1::2].sum())


def to_bbox(rle):
    """pycocotools' `toBbox`: [x, y, w, h] of the set pixels as floats, all zero for an empty mask"""
    H, W = rle["size"]
    counts = string_to_counts(rle["counts"])
    ends = np.cumsum(counts)
    s, e = (ends - counts)[1::2], ends[1::2] - 1          # first and last pixel of every run of ones
    keep = e >= s
    s, e = s[keep], e[keep]
    if len(s) == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, xe = s // H, e // H
    x1, x2 = int(xs.min()), int(xe.max())
    if (xe > xs).any():                                     # a run that crosses a column boundary touches the last and the first row
        y1, y2 = 0, H - 1
    else:
        y1, y2 = int((s % H).min()), int((e % H).max())
    return [float(x1), float(y1), float(x2 - x1 + 1), float(y2 - y1 + 1)]


# ---------------------------------------------------------------------------------------------------------------- on the device
def _two_pass(launch, K, H, W, device):
    """measure -> sizes to the host -> packed write -> characters to the host; `launch(sizes, offsets, chars, capacity)` enqueues a pass"""
    import torch
    sizes = torch.empty((K, 2), dtype=torch.int64, device=device)
    launch(sizes, None, None, 0)
    nchars = sizes[:, 1].cpu().numpy()                                       # device-to-host read 1: K pairs
    offsets = np.concatenate([[0], np.cumsum(nchars)]).astype(np.int64)
    total = int(offsets[-1])
    chars = torch.empty((total,), dtype=torch.uint8, device=device)
    launch(None, torch.from_numpy(offsets[:-1].copy()).to(device), chars, total)
    text = chars.cpu().numpy().tobytes().decode("ascii")                     # device-to-host read 2: the packed strings
    return [{"size": [int(H), int(W)], "counts": text[offsets[k]:offsets[k + 1]]} for k in range(K)]


def encode(masks):
    """device u8 / bool masks [K,H,W] or [H,W] (0 = clear) -> list of K records (one record for [H,W])"""
    import torch
    from . import _lib as L
    from .ops import _need_gpu, _p, _stream
    _need_gpu(masks)
    single = masks.dim() == 2
    m = masks[None] if single else masks
    assert m.dim() == 3 and m.dtype in (torch.uint8, torch.bool), "masks: [K,H,W] or [H,W], u8 or bool"
    m = m.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    K, H, W = m.shape
    if K == 0:
        return []

    def launch(sizes, offsets, chars, cap):
        L.check(L.lib().umr_rle_encode(_p(m), K, H, W, _p(sizes), _p(offsets), _p(chars), cap, _stream()), "umr_rle_encode")
    out = _two_pass(launch, K, H, W, m.device)
    return out[0] if single else out


def encode_pasted(sdf, center, int_boxes, select, H, W):
    """the records of the pasted union masks `umr_mask_paste` would write for the proposals `select` (int64 indices into the N proposals),
    without writing the masks: sdf [N,S,S] f32, center [N,2,S,S] f32, int_boxes [N,4] i32 (x1,y1,x2,y2 clipped to the image), all on the device"""
    import torch
    from . import _lib as L
    from .ops import _need_gpu, _p, _stream
    _need_gpu(sdf, center, int_boxes, select)
    assert sdf.dtype == torch.float32 and center.dtype == torch.float32 and int_boxes.dtype == torch.int32 and select.dtype == torch.int64
    sdf, center, int_boxes, select = sdf.contiguous(), center.contiguous(), int_boxes.contiguous(), select.contiguous()
    K, S = len(select), sdf.shape[-1]
    if K == 0:
        return []

    def launch(sizes, offsets, chars, cap):
        L.check(L.lib().umr_mask_paste_rle(_p(sdf), _p(center), _p(int_boxes), _p(select), K, S, H, W, _p(sizes), _p(offsets), _p(chars), cap,
                                           _stream()), "umr_mask_paste_rle")
    return _two_pass(launch, K, H, W, sdf.device)
