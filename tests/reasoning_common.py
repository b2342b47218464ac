"""Plain CPU restatements of the object-reasoning kernels (unmore_amd/csrc/reasoning.hip) -- union mask, erosion, anti-centre scores, peak
picking, the peak certificate, boundary box deltas, connected components, crop + resize -- written from the kernels' header comments and
oracle/objectness_oracle.py, for ANY (border, erode_kernel, erode_rounds) and map size, plus the builders of the constructed inputs the
GPU tests use.  tests/test_reasoning_kernels_cpu.py pins the restatements (to the oracle at the one configuration the oracle knows, to
hand-worked cases, to scipy) and proves that every constructed input does what it is for; tests/test_reasoning_kernels_gpu.py holds the
kernels to them.  No GPU is used here.

Error bounds.  u = 2^-24 (half a float32 ulp at 1), U53 = 2^-53.

Scores (peak_scores).  The kernel and this file add the same <= 50 float64 products in the same order (channel, filter row, filter
column) and divide by 24.  The products are exact in float64 (24-bit x 24-bit mantissas... the filter is a float32 value promoted), so
the only difference is that the compiler may contract `acc += a * b` into a fused multiply-add, which is not an error of either side but
moves the last bits: a chain of 50 additions and the division, each within U53 relative of a partial sum that is at most sum |a b|,
gives |device - restatement| <= 52 U53 sum |tap products| / 24 per pixel (score_bound, computed with the scores).

Boundary deltas (boundary_delta_intervals).  Per pixel of the (H-1) x (W-1) interior the kernel forms, in float32,
        dy, dx (one subtraction each: correctly rounded, identical on both sides), nr = sqrtf(dy dy + dx dx),
        fg = 1 / (1 + expf(-v)), bg = 1 - fg
and four sums of non-negative terms: s_fg = sum fg nr, s_bg = sum bg nr, n_fg = sum fg, n_bg = sum bg.  Every float32 elementwise
operation is taken to be within 1 ulp = 2 u relative (the correctly rounded ones are within u; the fused form of dy dy + dx dx is covered).
expf is taken within EXPF_ULP = 1 ulp: the figure of the HIP math API documentation (maximum ulp error of expf), NOT measured here.
  nr:  two products, an addition, the root: within 4 ulp = 8 u of the exact norm of (dy, dx)
  fg:  expf (1 ulp; its error reaches 1 + e^-v with a factor <= 1), the addition, the division: within 3 ulp = 6 u of sigmoid(v)
  fg nr: one more product on the device (2 u); the restatement multiplies exactly in float64.
So a device term of s_fg is within 16 u of the exact term, the restatement's within 14 u: they differ by at most 30 u relative (12 u for
n_fg); C_ELEM = 32 covers both and the products of the error terms.  A thread adds its ceil(n / 256) terms in a chain, the tree adds 8
levels, every addition within u of a non-negative partial sum; the restatement sums in float64.  With n = (H-1)(W-1):
        relative error of a sum of non-negative terms <= rel(n) = (1 + u)^(ceil(n / 256) + 8 + C_ELEM) - 1
bg = 1 - fg is NOT relatively accurate (fg -> 1): fg is within 6 u absolute (fg <= 1), the subtraction within 2 u, on each side, so the two
bg differ by at most A_BG = 16 u absolute per term.  The bg sums are therefore bounded as
        n_bg in [n_bg (1 - rel) - n A_BG, n_bg (1 + rel) + n A_BG (1 + rel)],   s_bg the same with sum nr (1 + 8 u) in the place of n
(clamped at 0: the terms are non-negative).  These four intervals go through the closed formula in float64:
        avg = s / (n + 1e-8f), step = 1 / (avg + 1e-10f)           step falls with s and rises with n: evaluated at the extremes;
        movement(y, x) = (step_fg fg + step_bg bg) v               per edge pixel: fg within 6 u relative, bg within A_BG absolute;
        delta = -max / -max / max / max over the left column, top row, right column, bottom row of the interior.
The float32 tail on the device (two additions and two divisions per step, two products, an addition and a product per movement: 9
operations, TAIL = 18 u charged) widens each movement interval outwards; the maximum of intervals is the interval of the maxima.
The device value must lie inside [lo, hi].  At 128 x 128 rel = 104 u = 6.2e-6: on the object fields the half width of the interval is
about 1e-5 of the delta (printed by the tests next to the observed error), below the 1e-4 + 1e-4 |ref| of tests/test_reasoning_gpu.py.
On a constant map the gradient is exactly 0 on both sides, the sums s are exactly 0 and step = 1 / 1e-10f: the interval there has only
the width of the tail and of fg / bg.  A saturated map (+-50) has fg == 1, bg == 0 exactly where v = 50; the absolute term A_BG keeps
the bound honest there (step_bg A_BG |v| is what a device whose fg were one ulp below 1 would add).

Crop + resize (crop_resize): the kernel's tap arithmetic op by op in numpy float32.  The source coordinate scale * (o + 0.5) - 0.5 is
written as the single-rounding fused multiply-add the compiler makes of it (an unfused coordinate differs by up to an ulp OF THE
COORDINATE, which moves the output by ulp(coordinate) * |tap difference| -- far more than the blend's own rounding at coordinates above
1 -- and the reference's CPU kernel, through the oracle, agrees with the fused form).  The blend itself is left unfused here; the tests
allow 4 float32 ulp of the largest of the four taps per output pixel for its contracted forms."""
import math

import numpy as np
import torch

U = 2.0 ** -24
U53 = 2.0 ** -53
EXPF_ULP = 1          # HIP math API documentation: expf, maximum error 1 ulp (taken from the documentation, not measured)
C_ELEM = 32           # elementwise error of one term of a sum, device against restatement, in units of u (module docstring)
A_BG = 16 * U         # absolute difference of the two sides' bg = 1 - fg
TAIL = 18             # float32 operations after the sums, in units of u
SQRT2 = math.sqrt(2.0)


def _np(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def anti_center_filter():
    """normalize((2-i, 2-j)) per tap in float32, promoted to float64 -- as unmore_amd.reasoning._anti_center_filter builds it."""
    g = np.zeros((2, 5, 5), np.float32)
    for i in range(5):
        for j in range(5):
            v = np.array([2 - i, 2 - j], np.float32)
            n = np.float32(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1])))
            g[:, i, j] = v / max(n, np.float32(1e-12))
    return g.astype(np.float64)


def _sigmoid32(s):
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32))).numpy()


def center_norm32(cen):
    c = _np(cen, np.float32)
    return np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1])          # float32 throughout


def union_mask(sdf, cen):
    """(sigmoid(s) > 0.5 in float32) | (sqrt(c0 c0 + c1 c1) > 0.5 in float32): [B,H,W] bool."""
    s = _np(sdf, np.float32)
    return (_sigmoid32(s) > np.float32(0.5)) | (center_norm32(cen) > np.float32(0.5))


def erode(mask, k, rounds):
    """zero-padded k x k all-ones erosion (keep a pixel when its whole k x k window is set), `rounds` times.  mask [..., H, W] bool."""
    assert k >= 1 and k % 2 == 1 and rounds >= 0
    m = np.asarray(mask, dtype=bool)
    r = (k - 1) // 2
    H, W = m.shape[-2:]
    for _ in range(rounds):
        p = np.zeros(m.shape[:-2] + (H + 2 * r, W + 2 * r), dtype=bool)
        p[..., r:r + H, r:r + W] = m
        out = np.ones_like(m)
        for dy in range(k):
            for dx in range(k):
                out &= p[..., dy:dy + H, dx:dx + W]
        m = out
    return m


def inside_border(H, W, border):
    ins = np.zeros((H, W), dtype=bool)
    if H - border > border and W - border > border:
        ins[border:H - border, border:W - border] = True
    return ins


def peak_scores(cen, mask, border, with_bound=False):
    """float64 5 x 5 correlation of the centre field with the anti-centre filter (zero padded), accumulated channel, filter row, filter
    column, then / 24; zero outside `mask` (the eroded mask, [B,H,W] bool) and within `border` pixels of the map's edge (border = 0: no
    edge strip).  with_bound: also the per-pixel bound 52 U53 sum |tap products| / 24 (module docstring)."""
    c = _np(cen, np.float32).astype(np.float64)
    B, _, H, W = c.shape
    f = anti_center_filter()
    p = np.zeros((B, 2, H + 4, W + 4), np.float64)
    p[:, :, 2:2 + H, 2:2 + W] = c
    acc = np.zeros((B, H, W), np.float64)
    mag = np.zeros((B, H, W), np.float64)
    for ch in range(2):
        for fi in range(5):
            for fj in range(5):
                t = p[:, ch, fi:fi + H, fj:fj + W] * f[ch, fi, fj]
                acc = acc + t
                mag = mag + np.abs(t)
    live = np.asarray(mask, dtype=bool) & inside_border(H, W, border)[None]
    score = np.where(live, acc / 24.0, 0.0)
    if with_bound:
        return score, np.where(live, 52.0 * U53 * mag / 24.0, 0.0)
    return score


def peak_pick(sdf, cen, border=10, k=9, rounds=3, with_bound=False):
    """(score maps [B,H,W] f64, max [B] f64, first flat argmax [B] int64[, score bound]) for any configuration."""
    er = erode(union_mask(sdf, cen), k, rounds)
    res = peak_scores(cen, er, border, with_bound)
    score = res[0] if with_bound else res
    flat = score.reshape(score.shape[0], -1)
    arg = flat.argmax(axis=1).astype(np.int64)          # numpy: the first maximum
    out = (score, flat[np.arange(len(arg)), arg].copy(), arg)
    return out + (res[1],) if with_bound else out


def flip_mask(sdf, cen, eps):
    """pixels whose union-mask decision a perturbation below eps can flip (center_peaks_cert_kernel: float32 distances, float32 eps)."""
    s = _np(sdf, np.float32)
    nr = center_norm32(cen)
    sb, cb = _sigmoid32(s) > np.float32(0.5), nr > np.float32(0.5)
    ds, dc = np.abs(s), np.abs(nr - np.float32(0.5))
    flip = np.where(sb & cb, np.maximum(ds, dc), np.where(sb, ds, np.where(cb, dc, np.minimum(ds, dc))))
    return flip < np.float32(eps)


def cert_bound(eps):
    return 2.0 * 1.4142135623730951 * float(np.float32(eps))


def peak_certificate(sdf, cen, eps, thres=0.009, border=10, k=9, rounds=3, with_branch=False):
    """center_peaks_cert_kernel's header, literally.  Returns (max [B], argmax [B], certified [B] bool[, branch names]).
    branch: 'cert_peak' | 'unc_runner' | 'unc_thres' | 'unc_min_mask' | 'cert_empty' | 'unc_empty' (the first failing clause, in the
    order smallest mask, runner-up, threshold)."""
    u = union_mask(sdf, cen)
    Fm = flip_mask(sdf, cen, eps)
    B, H, W = u.shape
    HW = H * W
    er = erode(u, k, rounds)
    er_min = erode(u & ~Fm, k, rounds)
    er_max = erode(u | Fm, k, rounds)
    score = peak_scores(cen, er, border)
    s_max = peak_scores(cen, er_max, border)                # exact zeros outside the largest mask and inside the border
    live_max = er_max & inside_border(H, W, border)[None]
    bound = cert_bound(eps)
    amax, arg = np.zeros(B), np.zeros(B, np.int64)
    cert = np.zeros(B, dtype=bool)
    branch = []
    for b in range(B):
        flat = score[b].reshape(-1)
        p = int(flat.argmax())
        a = float(flat[p])
        amax[b], arg[b] = a, p
        if a > 0.0:
            others = s_max[b].reshape(-1).copy()
            others[p] = -1.0e300
            runner = float(others.max()) if HW > 1 else -1.0e300
            in_min = bool(er_min[b].reshape(-1)[p])
            beats = a - runner > bound
            side = abs(a - thres) > bound
            cert[b] = in_min and beats and side
            branch.append("cert_peak" if cert[b] else "unc_min_mask" if not in_min else "unc_runner" if not beats else "unc_thres")
        else:
            lv = live_max[b]
            quiet = (not lv.any()) or float(s_max[b][lv].max()) < -bound
            cert[b] = a == 0.0 and p == 0 and border >= 1 and quiet and abs(thres) > bound
            branch.append("cert_empty" if cert[b] else "unc_empty")
    return (amax, arg, cert, branch) if with_branch else (amax, arg, cert)


# ---------------------------------------------------------------------------------------------------------------- boundary deltas
def _delta_parts(sdf):
    s = _np(sdf, np.float32)
    v = s[:, :-1, :-1]
    dy, dx = s[:, 1:, :-1] - v, s[:, :-1, 1:] - v
    nr = np.sqrt(dy * dy + dx * dx)                       # float32
    fg = _sigmoid32(v)
    bg = np.float32(1.0) - fg
    return v.astype(np.float64), nr.astype(np.float64), fg.astype(np.float64), bg.astype(np.float64)


E8, E10 = float(np.float32(1e-8)), float(np.float32(1e-10))


def _step(s, n):
    return 1.0 / (s / (n + E8) + E10)


def _edges(mv):
    """[B,h1,w1] movement -> [B,4] (-max left column, -max top row, max right column, max bottom row)"""
    return np.stack([-mv[:, :, 0].max(axis=1), -mv[:, 0, :].max(axis=1), mv[:, :, -1].max(axis=1), mv[:, -1, :].max(axis=1)], 1)


def boundary_deltas(sdf):
    """object_reasoning.py:139-174: float32 gradient norm, fg = sigmoid(v), bg = 1 - fg; float64 sums and float64 formula.  [B,4] f64."""
    v, nr, fg, bg = _delta_parts(sdf)
    sf, sb = _step((fg * nr).sum((1, 2)), fg.sum((1, 2))), _step((bg * nr).sum((1, 2)), bg.sum((1, 2)))
    return _edges((sf[:, None, None] * fg + sb[:, None, None] * bg) * v)


def boundary_delta_intervals(sdf, depth=None):
    """(ref [B,4], lo [B,4], hi [B,4]): the restatement and the interval a correct float32 kernel's deltas lie in (module docstring).
    depth: the number of additions a term of a sum passes through; default: the kernel's ceil(n / 256) + 8."""
    v, nr, fg, bg = _delta_parts(sdf)
    n = v.shape[1] * v.shape[2]
    rel = (1.0 + U) ** ((math.ceil(n / 256) + 8 if depth is None else depth) + C_ELEM) - 1.0
    s_fg, n_fg, s_bg, n_bg = (fg * nr).sum((1, 2)), fg.sum((1, 2)), (bg * nr).sum((1, 2)), bg.sum((1, 2))
    a_s, a_n = A_BG * nr.sum((1, 2)) * (1 + 8 * U), A_BG * n
    lohi = lambda x, a: (np.maximum(x * (1 - rel) - a, 0.0), x * (1 + rel) + a * (1 + rel))
    (sf_l, sf_h), (nf_l, nf_h) = lohi(s_fg, 0.0), lohi(n_fg, 0.0)
    (sb_l, sb_h), (nb_l, nb_h) = lohi(s_bg, a_s), lohi(n_bg, a_n)
    step_f = (_step(sf_h, nf_l), _step(sf_l, nf_h))
    step_b = (_step(sb_h, nb_l), _step(sb_l, nb_h))
    fg_l, fg_h = fg * (1 - 6 * U), fg * (1 + 6 * U)
    bg_l, bg_h = np.maximum(bg - A_BG, 0.0), bg + A_BG
    c_l = step_f[0][:, None, None] * fg_l + step_b[0][:, None, None] * bg_l
    c_h = step_f[1][:, None, None] * fg_h + step_b[1][:, None, None] * bg_h
    t = (1.0 + U) ** TAIL
    m_l = np.where(v >= 0, c_l * v / t, c_h * v * t)
    m_h = np.where(v >= 0, c_h * v * t, c_l * v / t)
    e_l, e_h = _edges(m_l), _edges(m_h)                    # columns 0, 1 are negated maxima: their ends swap
    lo = np.concatenate([e_h[:, :2], e_l[:, 2:]], 1)
    hi = np.concatenate([e_l[:, :2], e_h[:, 2:]], 1)
    return boundary_deltas(sdf), lo, hi


# ---------------------------------------------------------------------------------------------------------------- components
def components(mask):
    """8-connected components of one [S,S'] bool mask by flood fill from every unvisited pixel in raster order.
    Returns (count, boxes [count,4] int32 [x1,y1,x2,y2)) in first-pixel order."""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape
    seen = np.zeros_like(m)
    boxes = []
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack = [(y0, x0)]
            x1 = x2 = x0
            y1 = y2 = y0
            while stack:
                y, x = stack.pop()
                x1, x2, y1, y2 = min(x1, x), max(x2, x), min(y1, y), max(y2, y)
                for yy in range(max(y - 1, 0), min(y + 2, H)):
                    for xx in range(max(x - 1, 0), min(x + 2, W)):
                        if m[yy, xx] and not seen[yy, xx]:
                            seen[yy, xx] = True
                            stack.append((yy, xx))
            boxes.append((x1, y1, x2 + 1, y2 + 1))
    return len(boxes), np.asarray(boxes, dtype=np.int32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------------------------- crop + resize
def crop_resize(image, int_boxes, S, with_taps=False):
    """crop_resize_kernel's arithmetic op by op in numpy float32: the `area_pixel` source index scale * (o + 0.5) - 0.5 clamped at 0,
    the index clamp to the crop, weights l and 1 - l, out = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11).  image [3,H,W] f32,
    int_boxes [N,4] integer corners inside the image; an empty box gives zeros.  with_taps: also the largest |tap| per output pixel, the
    (clamped) float32 source coordinates (sy [N,S], sx [N,S]) and where the blend is exact in float32 at every step."""
    img = _np(image, np.float32)
    f = np.float32
    N = len(int_boxes)
    out = np.zeros((N, 3, S, S), np.float32)
    big = np.zeros((N, 3, S, S), np.float32)
    exact = np.zeros((N, 3, S, S), bool)
    SY, SX = np.zeros((N, S), np.float32), np.zeros((N, S), np.float32)
    o = np.arange(S, dtype=np.float32) + f(0.5)
    for n, (x1, y1, x2, y2) in enumerate(np.asarray(int_boxes, dtype=np.int64).tolist()):
        hc, wc = y2 - y1, x2 - x1
        if hc <= 0 or wc <= 0:
            continue
        sh, sw = f(hc) / f(S), f(wc) / f(S)
        # scale * (o + 0.5) - 0.5 is ONE fused multiply-add in the built kernel (and in the reference's CPU kernel, which the oracle
        # runs): the product is exact in float64 (24 x 24 bits), the subtraction of 0.5 too, so this rounds once, like the fma
        fma = lambda a: (a.astype(np.float64) * o.astype(np.float64) - 0.5).astype(np.float32)
        sy, sx = np.maximum(fma(sh), f(0)), np.maximum(fma(sw), f(0))
        iy, ix = np.minimum(sy.astype(np.int64), hc - 1), np.minimum(sx.astype(np.int64), wc - 1)
        dy, dx = (iy < hc - 1).astype(np.int64), (ix < wc - 1).astype(np.int64)
        ly1 = np.clip(sy - iy.astype(np.float32), f(0), f(1))
        lx1 = np.clip(sx - ix.astype(np.float32), f(0), f(1))
        ly0, lx0 = f(1) - ly1, f(1) - lx1
        Y0, Y1, X0, X1 = y1 + iy, y1 + iy + dy, x1 + ix, x1 + ix + dx
        v00, v01 = img[:, Y0[:, None], X0[None, :]], img[:, Y0[:, None], X1[None, :]]
        v10, v11 = img[:, Y1[:, None], X0[None, :]], img[:, Y1[:, None], X1[None, :]]
        LX0, LX1, LY0, LY1 = lx0[None, None, :], lx1[None, None, :], ly0[None, :, None], ly1[None, :, None]
        out[n] = LY0 * (LX0 * v00 + LX1 * v01) + LY1 * (LX0 * v10 + LX1 * v11)
        # where NO step of the blend rounds (float64 shadow == its float32 rounding at every step), any contraction gives the same bits
        d = np.float64
        fits = lambda a: a.astype(np.float32).astype(d) == a
        ok = fits(1.0 - ly1.astype(d))[None, :, None] & fits(1.0 - lx1.astype(d))[None, None, :]
        rows = []
        for (va, vb) in ((v00, v01), (v10, v11)):
            pa, pb = LX0.astype(d) * va.astype(d), LX1.astype(d) * vb.astype(d)
            ok = ok & fits(pa) & fits(pb) & fits(pa + pb)
            rows.append(pa + pb)
        qa, qb = LY0.astype(d) * rows[0], LY1.astype(d) * rows[1]
        exact[n] = ok & fits(qa) & fits(qb) & fits(qa + qb)
        big[n] = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
        SY[n], SX[n] = np.minimum(sy, f(hc - 1)), np.minimum(sx, f(wc - 1))
    return (out, big, SY, SX, exact) if with_taps else out


# ---------------------------------------------------------------------------------------------------------------- constructed inputs
PEAK_SHAPES = [(1, 1), (5, 7), (16, 16), (23, 37), (40, 64)]
PEAK_CONFIGS = [(0, 5, 0), (0, 1, 1), (2, 3, 1), (2, 3, 2), (10, 9, 3)]          # (border, erode_kernel, erode_rounds)
PEAK_CASES = [(H, W, cfg) for (H, W) in PEAK_SHAPES for cfg in PEAK_CONFIGS] + [(240, 320, (10, 9, 3))]
PEAK_B = 4                # maps per case (even: converging, odd: diverging); the LDS-limit case has one
PEAK_SEED = 11


def object_fields(B, H, W, seed):
    """tests/test_reasoning_gpu.py::_fields with centres, radii and the edge softness relative to the map: two discs per map, unit
    vectors converging on (even maps) or diverging from (odd maps) the disc centres, 0.05 noise."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    sdf = torch.zeros(B, H, W)
    cen = torch.zeros(B, 2, H, W)
    soft = max(min(H, W) / 16.0, 0.5)
    for b in range(B):
        for _ in range(2):
            cy, cx = (0.25 + 0.5 * torch.rand(2, generator=g)) * torch.tensor([H, W])
            r = (0.15 + 0.2 * torch.rand(1, generator=g)) * min(H, W)
            d = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            sdf[b] = torch.maximum(sdf[b], torch.tanh((r - d) / soft))
            inside = d < r
            n = d + 1e-6
            sign = -1.0 if b % 2 == 0 else 1.0
            cen[b, 0] = torch.where(inside, sign * (yy - cy) / n, cen[b, 0])
            cen[b, 1] = torch.where(inside, sign * (xx - cx) / n, cen[b, 1])
        sdf[b] = sdf[b] * 2 - 0.3
    sdf += 0.05 * torch.randn(B, H, W, generator=g)
    cen += 0.05 * torch.randn(B, 2, H, W, generator=g)
    return sdf, cen


def peak_case_fields(H, W):
    return object_fields(1 if H * W > 40 * 64 else PEAK_B, H, W, PEAK_SEED + H * 1000 + W)


# the cases whose converging map (index 0) must have a positive peak -- proven by tests/test_reasoning_kernels_cpu.py
POSITIVE_PEAK_CASES = [(H, W, cfg) for (H, W, cfg) in PEAK_CASES
                       if (min(H, W) >= 16 and cfg != (10, 9, 3)) or (min(H, W) >= 240)]


def converging_patch(n=11):
    """[2,n,n] unit vectors pointing at the patch centre (zero there): an isolated positive anti-centre peak at the centre."""
    c = (n - 1) / 2.0
    yy, xx = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    d = np.sqrt((yy - c) ** 2 + (xx - c) ** 2).astype(np.float32)
    d[d == 0] = 1
    return np.stack([-(yy - np.float32(c)) / d, -(xx - np.float32(c)) / d]).astype(np.float32)


# name -> (H, W, (y, x) of the two patch centres): flat indices i1 < i2; 'cross': i2 % 256 < i1 % 256 (the later pixel sits in the lower
# thread), 'same': i1 % 256 == i2 % 256 (one thread owns both)
TIE_CASES = {"cross": (40, 64, (9, 40), (24, 10)), "same": (40, 64, (9, 40), (25, 40))}
TIE_CONFIG = (2, 3, 1)


def tie_fields(name):
    """two bit-identical 11 x 11 converging patches on a zero centre field, sdf = +1 over both (-1 elsewhere).  Returns (sdf [1,H,W],
    cen [1,2,H,W], i1, i2): the flat indices of the two patch centres."""
    H, W, p1, p2 = TIE_CASES[name]
    sdf = -np.ones((1, H, W), np.float32)
    cen = np.zeros((1, 2, H, W), np.float32)
    pt = converging_patch(11)
    for (y, x) in (p1, p2):
        cen[0, :, y - 5:y + 6, x - 5:x + 6] = pt
        sdf[0, y - 5:y + 6, x - 5:x + 6] = 1.0
    return torch.from_numpy(sdf), torch.from_numpy(cen), p1[0] * W + p1[1], p2[0] * W + p2[1]


def diverging_full_mask(H=3, W=4):
    """a unit field diverging from a point near the centre of a map so small that every pixel sees that point inside its 5 x 5 window,
    under a full mask (sdf = +1): every score is negative, also at the edges (on a larger map the zero padding makes edge scores
    positive).  The point is off the pixel grid, so no two scores are alike."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cy, cx = np.float32((H - 1) / 2 + 0.13), np.float32((W - 1) / 2 - 0.21)
    d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2).astype(np.float32)
    cen = np.stack([(yy - cy) / d, (xx - cx) / d])[None].astype(np.float32)
    return torch.ones(1, H, W), torch.from_numpy(cen)


CERT_EPS_VALUES = [0.0, 2e-4, 5e-2]
CERT_CONFIG = (2, 3, 1)


def certificate_cases():
    """name -> (sdf, cen, eps, thres, (border, k, rounds), intended branch).  40 x 64 maps at CERT_CONFIG; a patch is an 11 x 11
    converging (or diverging) field of norm 0.4 -- below the centre half of the union mask, 0.1 away from its threshold -- with sdf = +1 on
    the 3 x 3 pixels round its centre only, so that exactly the patch centre survives the erosion, in all three masks, and is the only
    scored pixel: peak 0.4 scale, everything else exactly 0.  Thresholds beside a maximum are computed from the restatement.  Proven to
    land in their branches by tests/test_reasoning_kernels_cpu.py."""
    cases = {}
    cfg = CERT_CONFIG
    H, W = 40, 64
    pt = converging_patch(11) * np.float32(0.4)

    def patches(scale1=1.0, scale2=None, sdf_in=1.0):
        sdf = -np.ones((1, H, W), np.float32)
        cen = np.zeros((1, 2, H, W), np.float32)
        cen[0, :, 10:21, 12:23] = pt * np.float32(scale1)
        sdf[0, 14:17, 16:19] = sdf_in
        if scale2 is not None:                      # a second, weaker peak: the runner-up
            cen[0, :, 22:33, 40:51] = pt * np.float32(scale2)
            sdf[0, 26:29, 44:47] = sdf_in
        return torch.from_numpy(sdf), torch.from_numpy(cen)

    bg = (-torch.ones(1, H, W), torch.zeros(1, 2, H, W))
    for eps in CERT_EPS_VALUES:
        tag = f"eps{eps:g}"
        bound = cert_bound(eps)
        s, c = patches(scale2=0.5)
        mx = float(peak_pick(s, c, *cfg)[1][0])
        for thres in (0.009, 0.05):
            cases[f"peak_{tag}_thres{thres:g}"] = (s, c, eps, thres, cfg, "cert_peak")
        if eps > 0:
            cases[f"thres_inside_{tag}"] = (s, c, eps, mx + 0.9 * bound, cfg, "unc_thres")
            cases[f"thres_outside_{tag}"] = (s, c, eps, mx + 1.1 * bound, cfg, "cert_peak")
            # the peak pixel's own mask decision can flip: sdf inside eps of 0 there, centre norm below 0.5
            s3, c3 = patches(sdf_in=0.5 * eps)
            cases[f"min_mask_{tag}"] = (s3, c3, eps, 0.009, cfg, "unc_min_mask")
        # runner-up within the bound: the second peak half a bound below the first (eps = 0: an exact tie, the one thing it cannot beat)
        s2, c2 = patches(scale2=1.0 - 0.5 * bound / mx)
        cases[f"runner_{tag}"] = (s2, c2, eps, 0.009, cfg, "unc_runner")
        # no peak: one diverging patch (score -0.4, well below every bound) or background only; certified while |thres| > bound
        s4, c4 = patches(scale1=-1.0)
        for thres in (0.009, 0.5):
            want = "cert_empty" if abs(thres) > bound else "unc_empty"
            cases[f"empty_neg_{tag}_thres{thres:g}"] = (s4, c4, eps, thres, cfg, want)
            cases[f"empty_bg_{tag}_thres{thres:g}"] = bg + (eps, thres, cfg, want)
        if eps > 0:
            cases[f"empty_small_thres_{tag}"] = bg + (eps, 0.5 * bound, cfg, "unc_empty")      # |thres| < bound on an empty map
            # a diverging patch so weak that a perturbation could lift its score above zero
            s5, c5 = patches(scale1=-0.25 * bound / mx)
            cases[f"empty_weak_{tag}"] = (s5, c5, eps, 0.5, cfg, "unc_empty")
        # border == 0: the no-peak branch must not certify (index 0 is no border pixel)
        cases[f"empty_border0_{tag}"] = bg + (eps, 0.5, (0, 3, 1), "unc_empty")
    # H * W == 1: the only tap is the centre one, whose filter value is 0: score 0, and border == 0 certifies nothing
    cases["one_pixel"] = (torch.ones(1, 1, 1), torch.ones(1, 2, 1, 1), 2e-4, 0.009, (0, 1, 0), "unc_empty")
    return cases


# ---- component masks
def component_masks(S):
    """name -> [S,S] bool."""
    m = {}
    m["empty"] = np.zeros((S, S), bool)
    m["full"] = np.ones((S, S), bool)
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, S - 1), "corner_bl": (S - 1, 0), "corner_br": (S - 1, S - 1)}.items():
        a = np.zeros((S, S), bool)
        a[y, x] = True
        m[name] = a
    m["diag_down"] = np.eye(S, dtype=bool)
    m["diag_up"] = np.eye(S, dtype=bool)[::-1].copy()
    a = np.zeros((S, S), bool)                     # one-pixel serpentine: full rows 0, 2, 4, ... joined alternately right and left
    for y in range(0, S, 2):
        a[y, :] = True
        if y + 1 < S:
            a[y + 1, S - 1 if (y // 2) % 2 == 0 else 0] = True
    if S % 2 == 0:
        a[S - 1, :] = False                        # (the last joint would dangle: drop it)
    m["serpentine"] = a
    a = np.zeros((S, S), bool)                     # nested rings, two pixels apart: separate components, outermost first
    for r in range(0, (S + 1) // 2, 2):
        a[r, r:S - r] = a[S - 1 - r, r:S - r] = True
        a[r:S - r, r] = a[r:S - r, S - 1 - r] = True
    m["rings"] = a
    a = np.zeros((S, S), bool)
    a[::2, ::2] = True
    m["isolated"] = a
    return m


def mask_to_fields(mask, via_center=False):
    """[S,S] bool -> (sdf [1,S,S], cen [1,2,S,S]) whose union mask is `mask`, switched on by the sdf half or by the centre-field half."""
    m = torch.from_numpy(np.asarray(mask, dtype=bool))[None]
    if via_center:
        cen = torch.zeros(1, 2, *mask.shape)
        cen[:, 0] = torch.where(m, 0.6, 0.4)       # norms 0.6 / 0.4 either side of 0.5
        return -torch.ones(1, *mask.shape), cen
    return torch.where(m, 1.0, -1.0), torch.zeros(1, 2, *mask.shape)


# ---- crop + resize inputs
def ramp_images(H, W):
    """[3,H,W] float32 integers: x, y, x + y.  On a ramp the blend of a and a + 1 with weights (1 - l, l) is the source coordinate."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    return np.stack([xx, yy, xx + yy]).astype(np.float32)


def crop_boxes(H, W):
    """integer [x1,y1,x2,y2): a 1 x 1 crop, the whole image, a crop at each image corner, an odd interior crop, an empty box."""
    return [[5, 6, 6, 7], [0, 0, W, H], [0, 0, 9, 7], [W - 9, 0, W, 7], [0, H - 7, 9, H], [W - 9, H - 7, W, H], [3, 2, 22, 15], [5, 5, 5, 9]]


# ---- boundary-delta inputs
DELTA_SHAPES = [(2, 2), (2, 300), (300, 2), (17, 33), (128, 128)]


def delta_inputs(H, W):
    """name -> sdf [B,H,W] f32: object fields; constant maps (gradient exactly 0: step = 1 / 1e-10); maps saturated at +-50 (fg == 1 and
    bg == 0 exactly where v = 50) with both signs among the summed pixels; all-negative maps."""
    obj, _ = object_fields(3, H, W, 5 + H + W)
    const = torch.stack([torch.full((H, W), v) for v in (0.7, -0.3, 0.0)])
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sat = torch.stack([torch.where((xx + yy // 2) % 5 < 2, 50.0, -50.0), torch.where((xx * 3 + yy) % 7 < 4, -50.0, 50.0)])
    return {"object": obj, "constant": const, "saturated": sat, "negative": obj - 5.0}
