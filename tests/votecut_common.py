"""Shared by test_votecut_cpu.py / test_votecut_gpu.py: the mask patterns and the host checker of the largest 4-connected component."""
import numpy as np
from scipy import ndimage

SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 65), (64, 64), (150, 210)]
BIG = (375, 500)
ZERO_RUN_COUNTS = [3, 2, 0, 4, 0, 0, 5, 1, 0, 2, 7]      # zero-length runs in the middle: ones at 3-4 and 5-8 touch, then 14, then 15-16


def largest_numpy(mask):
    """[H,W] 0/non-zero -> (u8 mask of 0/255 holding the largest 4-connected component, (number of components, its area)).
    scipy.ndimage.label's default structure is the 4-neighbourhood and it numbers components by their first pixel in raster order;
    np.argmax takes the first maximum: ties go to the component whose first raster pixel comes first."""
    lab, n = ndimage.label(np.asarray(mask) != 0)
    if n == 0:
        return np.zeros(lab.shape, np.uint8), (0, 0)
    areas = np.bincount(lab.reshape(-1))[1:]
    k = int(np.argmax(areas))
    return ((lab == k + 1) * 255).astype(np.uint8), (int(n), int(areas[k]))


def zero_run_record(H, W):
    """an uncompressed record whose count list has zero-length runs in the middle; the rest of the mask is clear"""
    used = sum(ZERO_RUN_COUNTS)
    assert H * W >= used
    counts = list(ZERO_RUN_COUNTS)
    counts[-1] += H * W - used                   # the last run is one of zeros
    return {"size": [H, W], "counts": counts}


def counts_to_mask(counts, H, W):
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return flat.reshape((H, W), order="F")


def pattern(name, H, W, seed=0):
    """[H,W] u8 of 0/1"""
    m = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "empty":
        pass
    elif name == "full":
        m[:] = 1
    elif name == "checkerboard":
        m[:] = (yy + xx) & 1 ^ 1
    elif name == "stripes":                      # row stripes
        m[::2] = 1
    elif name == "noise":
        m[:] = np.random.default_rng(seed + 1000 * H + W).random((H, W)) < 0.55
    elif name in ("corner00", "corner01", "corner10", "corner11"):
        m[(H - 1) * int(name[6]), (W - 1) * int(name[7])] = 1
    elif name == "serpentine":                   # full even rows joined alternately at the right and the left end: one component
        m[::2] = 1
        for y in range(1, H, 2):
            m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    elif name == "serpentine_t":
        m = np.ascontiguousarray(pattern("serpentine", W, H).T)
    elif name == "u":                            # two columns that join only in the last row
        m[:, 0] = 1
        m[:, W - 1] = 1
        m[H - 1] = 1
    elif name == "comb":                         # every second column, joined only in the last row
        m[:, ::2] = 1
        m[H - 1] = 1
    elif name == "diagonal":                     # 8-connected, not 4-connected
        d = np.arange(min(H, W))
        m[d, d] = 1
    elif name == "tie":                          # two 2x2 blocks: top right (first in raster order) and bottom left (first in column-major order)
        m[:2, max(W - 2, 0):] = 1
        if H >= 5 and W >= 5:
            m[H - 2:, :2] = 1
    elif name == "wrap":                         # neighbours in the string, not in the image (for H > 1)
        x = max(W // 2 - 1, 0)
        m[H - 1, x] = 1
        m[0, min(x + 1, W - 1)] = 1
    else:
        raise KeyError(name)
    return m


DECODE_PATTERNS = ["empty", "full", "checkerboard", "stripes", "noise", "corner00", "corner01", "corner10", "corner11"]
LARGEST_PATTERNS = ["empty", "full", "checkerboard", "serpentine", "serpentine_t", "u", "comb", "diagonal", "tie", "wrap", "noise"]


def blob(H, W, seed):
    """a smoothed-noise blob mask (a few components, a few hundred runs), 0/1"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma=max(min(H, W) / 12.0, 1.0))
    return (f > np.quantile(f, 0.7)).astype(np.uint8)
