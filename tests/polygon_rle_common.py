"""What the polygon rasteriser's tests share: the C form of maskApi.c's rleFrPoly tail (sort, differences, zero counts folded) and
of rleMerge (the union of run-length masks, one run at a time), both restated sequentially, and seeded polygon generators.  The
arithmetic up to the crossings is unmore_amd.rle.polygon_crossings_numpy; pycocotools itself is not a dependency of this repository,
so parity with it is unpinned and rests on these restatements, which tests/test_polygon_rle_cpu.py pins on cases worked out by hand."""
import numpy as np

from unmore_amd import rle


def fr_poly_counts_c(xy, h, w):
    """rleFrPoly after the crossings: append h*w, sort, take differences, fold every zero difference (but the first) into its
    neighbours"""
    a = sorted(int(v) for v in rle.polygon_crossings_numpy(xy, h, w)) + [h * w]
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    k = len(a)
    b = [a[0]]
    j = 1
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def rle_merge_union(counts_list, h, w):
    """rleMerge(R, M, n, intersect=0): the masks are folded in one after the other, two run lists walked in step"""
    if len(counts_list) == 0:
        return []
    cnts = [int(c) for c in counts_list[0]]
    for B in counts_list[1:]:
        A = cnts
        B = [int(c) for c in B]
        ca, cb = A[0], B[0]
        v = va = vb = False
        out = []
        a = b = 1
        cc, ct = 0, 1
        while ct > 0:
            c = min(ca, cb)
            cc += c
            ct = 0
            ca -= c
            if not ca and a < len(A):
                ca = A[a]
                a += 1
                va = not va
            ct += ca
            cb -= c
            if not cb and b < len(B):
                cb = B[b]
                b += 1
                vb = not vb
            ct += cb
            vp = v
            v = va or vb
            if v != vp or ct == 0:
                out.append(cc)
                cc = 0
        cnts = out
    return cnts


def counts_of(record):
    return [int(c) for c in rle.string_to_counts(record["counts"])]


def parity_mask(seg, h, w):
    """the OR of the polygons' parity masks, [h, w] u8"""
    m = np.zeros((h, w), np.uint8)
    for xy in seg:
        m |= rle.polygon_mask_numpy(xy, h, w)
    return m


# ---------------------------------------------------------------------------------------------------------------- generators
def random_polygon(rng, h, w, k, mode, spread=0.3):
    """k vertices; mode 0 integer, 1 half-integer, 2 random coordinates; spread: how far beyond the image they may lie"""
    pts = np.stack([rng.uniform(-spread * w, (1 + spread) * w, k), rng.uniform(-spread * h, (1 + spread) * h, k)], axis=1)
    if mode == 0:
        pts = np.round(pts)
    elif mode == 1:
        pts = np.round(pts * 2) / 2
    return [float(v) for v in pts.reshape(-1)]


def ellipse(cx, cy, rx, ry, k, wobble=0.0, phase=0.0):
    t = phase + np.arange(k) * 2 * np.pi / k
    pts = np.stack([cx + rx * np.cos(t) + wobble * np.sin(7 * t), cy + ry * np.sin(t)], axis=1)
    return [float(v) for v in pts.reshape(-1)]


def sweep(h, w, n_edges):
    """a closed zigzag of n_edges (even) edges, each from beyond one side of the image to beyond the other: every edge steps over all
    w column lines, so the polygon has n_edges * w crossings"""
    assert n_edges % 2 == 0
    pts = []
    for i in range(n_edges):
        pts += [-2.0 if i % 2 == 0 else w + 2.0, 0.5 + (i * 0.37) % (h - 1)]
    return pts
