"""The object-reasoning kernels (unmore_amd/csrc/reasoning.hip: centre peaks, the peak certificate, boundary deltas, connected components,
crop + resize) against the plain restatements of tests/reasoning_common.py, at the configurations, map sizes and launch-plan edges the
feature tests never reach: any (border, erode_kernel, erode_rounds); H * W below, at and above the 256 threads of the one workgroup per
map; ragged strides; ties across and inside threads; maps without a scored pixel; maps at the LDS limit and one pixel over it.  The bounds
are derived in reasoning_common's docstring; tests/test_reasoning_kernels_cpu.py proves that the constructed inputs do what they are for.
Every family prints its number of cases and its largest observed error next to the derived bound (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import reasoning_common as rc

pytestmark = pytest.mark.gpu
REPORT = {}


def _cfg(cfg):
    return dict(border=cfg[0], erode_kernel=cfg[1], erode_rounds=cfg[2])


def _note(family, cases=1, excused=0, err=0.0, bound=0.0):
    r = REPORT.setdefault(family, dict(cases=0, excused=0, ratio=-1.0, err=0.0, bound=0.0))
    r["cases"] += cases
    r["excused"] += excused
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    if ratio > r["ratio"] or (ratio == r["ratio"] and bound > r["bound"]):
        r.update(ratio=ratio, err=err, bound=bound)


def _line(family):
    r = REPORT.get(family)
    if r:
        print(f"[reasoning kernels] {family}: {r['cases']} cases, {r['excused']} excused ties, largest error {r['err']:.3e} "
              f"at a derived bound of {r['bound']:.3e} (ratio {r['ratio']:.3f})")


# ------------------------------------------------------------------------------------------------------------------ center_peaks
@pytest.fixture(scope="module")
def peak_runs():
    """every case once: (restatement, device) per (H, W, configuration)"""
    from unmore_amd import reasoning
    runs = {}
    for (H, W, cfg) in rc.PEAK_CASES:
        sdf, cen = rc.peak_case_fields(H, W)
        ref = rc.peak_pick(sdf, cen, *cfg, with_bound=True)
        mx, am, sc = reasoning.center_peaks(sdf.cuda(), cen.cuda(), return_scores=True, **_cfg(cfg))
        runs[(H, W, cfg)] = (ref, mx.cpu().numpy(), am.cpu().numpy(), sc.cpu().numpy())
    return runs


def _check_peaks(ref, mx, am, sc, tag):
    """-> (number of maps whose argmax differs by a PROVEN tie, largest error, its bound)"""
    score, max_r, arg_r, bound = ref
    B = len(max_r)
    np.testing.assert_array_equal(sc != 0, score != 0)                                  # the integer side: identical support
    err = np.abs(sc - score)
    assert np.all(err <= bound), (tag, float((err - bound).max()))
    flat_d, flat_r, flat_b = sc.reshape(B, -1), score.reshape(B, -1), bound.reshape(B, -1)
    excused = 0
    for b in range(B):
        assert flat_d[b].argmax() == am[b] and flat_d[b, am[b]] == mx[b], (tag, b)      # the FIRST maximum of the device's own map
        if am[b] != arg_r[b]:
            gap = abs(flat_r[b, am[b]] - flat_r[b, arg_r[b]])
            print(f"[reasoning kernels] {tag} map {b}: argmax {int(am[b])} vs {int(arg_r[b])}, restated scores {gap:.3e} apart")
            assert gap <= 2 * max(flat_b[b, am[b]], flat_b[b, arg_r[b]]), (tag, b, gap)
            excused += 1
        assert abs(mx[b] - max_r[b]) <= flat_b[b, arg_r[b]] + (flat_b[b, am[b]] if am[b] != arg_r[b] else 0.0)
    i = np.unravel_index(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)), err.shape)
    if err[i] == 0:                                     # bit-identical scores: report the bound they would have been allowed
        i = np.unravel_index(np.argmax(bound), err.shape)
    return excused, float(err[i]), float(bound[i])


@pytest.mark.parametrize("H,W,cfg", rc.PEAK_CASES, ids=[f"{H}x{W}-b{c[0]}k{c[1]}r{c[2]}" for (H, W, c) in rc.PEAK_CASES])
def test_center_peaks_against_the_restatement(peak_runs, H, W, cfg):
    ref, mx, am, sc = peak_runs[(H, W, cfg)]
    tag = f"center_peaks {H}x{W} {cfg}"
    _check_peaks(ref, mx, am, sc, tag)
    if (H, W, cfg) in rc.POSITIVE_PEAK_CASES:
        assert mx[0] > 0
    if min(H, W) <= 2 * cfg[0]:                        # too small for the configuration: the pinned result
        assert np.all(mx == 0.0) and np.all(am == 0) and not sc.any()


def test_center_peaks_tie_excuses_stay_within_two_percent(peak_runs):
    maps = excused = 0
    for key, (ref, mx, am, sc) in peak_runs.items():
        e, err, bound = _check_peaks(ref, mx, am, sc, f"center_peaks {key}")
        maps += len(mx)
        excused += e
        _note("center_peaks", 1, e, err, bound)
    assert maps >= 100 and excused <= 0.02 * maps, (excused, maps)
    _line("center_peaks")


def _sentinels(B):
    return (torch.full((B,), -7.5, dtype=torch.float64, device="cuda"), torch.full((B,), -7, dtype=torch.int64, device="cuda"),
            torch.full((B,), -7, dtype=torch.int32, device="cuda"))


def test_center_peaks_one_pixel_over_the_lds_limit_is_refused_before_any_launch():
    """umr_center_peaks checks H * W * 2 <= 150 KiB before it launches (csrc/reasoning.hip): status, message, outputs untouched."""
    from unmore_amd import _lib as L, reasoning
    from unmore_amd.ops import _p, _stream
    H, W = 240, 321
    sdf, cen = torch.zeros(1, H, W, device="cuda"), torch.zeros(1, 2, H, W, device="cuda")
    mx, am, _ = _sentinels(1)
    st = L.lib().umr_center_peaks(_p(sdf), _p(cen), _p(reasoning._anti_center_filter(sdf.device)), None, _p(mx), _p(am), 1, H, W, 10, 9, 3, _stream())
    with pytest.raises(RuntimeError, match="larger than the LDS mask planes"):
        L.check(st, "umr_center_peaks")
    torch.cuda.synchronize()
    assert mx.item() == -7.5 and am.item() == -7
    with pytest.raises(RuntimeError, match="larger than the LDS mask planes"):
        reasoning.center_peaks(sdf, cen)


@pytest.mark.parametrize("name", list(rc.TIE_CASES))
def test_the_first_of_two_bit_equal_maxima_wins(name):
    from unmore_amd import reasoning
    sdf, cen, i1, i2 = rc.tie_fields(name)
    score, max_r, arg_r = rc.peak_pick(sdf, cen, *rc.TIE_CONFIG)
    mx, am, sc = reasoning.center_peaks(sdf.cuda(), cen.cuda(), return_scores=True, **_cfg(rc.TIE_CONFIG))
    flat = sc.cpu().numpy().reshape(-1)
    assert flat[i1] == flat[i2] == mx.item() > 0                  # bit-identical patches: the same instructions on the same values
    assert am.item() == i1 == arg_r[0]
    mx2, am2, ce = reasoning.center_peaks_certified(sdf.cuda(), cen.cuda(), 2e-4, **_cfg(rc.TIE_CONFIG))
    assert torch.equal(mx2, mx) and torch.equal(am2, am) and not bool(ce.item())
    _note("ties")


def test_all_negative_and_all_zero_maps():
    from unmore_amd import reasoning
    sdf, cen = rc.diverging_full_mask()
    ref = rc.peak_pick(sdf, cen, 0, 5, 0, with_bound=True)
    mx, am, sc = reasoning.center_peaks(sdf.cuda(), cen.cuda(), border=0, erode_kernel=5, erode_rounds=0, return_scores=True)
    e, err, bound = _check_peaks(ref, mx.cpu().numpy(), am.cpu().numpy(), sc.cpu().numpy(), "all negative")
    assert e == 0 and mx.item() < 0 and am.item() == ref[2][0] != 0            # the least negative score, not index 0
    _note("all-negative / all-zero", 1, 0, err, bound)
    mx, am, sc = reasoning.center_peaks(sdf.cuda(), cen.cuda(), border=2, erode_kernel=5, erode_rounds=0, return_scores=True)
    assert mx.item() == 0.0 and am.item() == 0 and not bool(sc.any())
    mx0, am0 = reasoning.center_peaks(sdf.cuda(), cen.cuda(), border=0, erode_kernel=5, erode_rounds=0)
    mxc, amc, ce = reasoning.center_peaks_certified(sdf.cuda(), cen.cuda(), 2e-4, border=0, erode_kernel=5, erode_rounds=0)
    assert torch.equal(mxc, mx0) and torch.equal(amc, am0) and amc.item() == ref[2][0] and not bool(ce.item())
    _note("all-negative / all-zero")
    _line("all-negative / all-zero")


# ------------------------------------------------------------------------------------------------------------------ certificate
def _certified(sdf, cen, eps, thres, cfg):
    """device (max, argmax, certified) with the plain kernel's (max, argmax) required bit for bit"""
    from unmore_amd import reasoning
    s, c = sdf.cuda(), cen.cuda()
    mx0, am0 = reasoning.center_peaks(s, c, **_cfg(cfg))
    mx, am, ce = reasoning.center_peaks_certified(s, c, eps, singular_threshold=thres, **_cfg(cfg))
    assert torch.equal(mx0, mx) and torch.equal(am0, am)
    return mx.cpu().numpy(), am.cpu().numpy(), ce.cpu().numpy()


def _compare_certificates(sdf, cen, eps, thres, cfg, tag):
    """border >= 1: the certified set equals the restatement's.  border == 0: a subset of it -- the kernel clamps a negative runner-up to 0
    even when no pixel lies outside the largest mask (no exact zero exists then); sound, but stricter than its header."""
    a_r, p_r, c_r = rc.peak_certificate(sdf, cen, eps, thres, *cfg)
    mx, am, ce = _certified(sdf, cen, eps, thres, cfg)
    np.testing.assert_array_equal(am, p_r, err_msg=tag)
    assert np.all(np.abs(mx - a_r) <= 1e-14), tag
    if cfg[0] >= 1:
        np.testing.assert_array_equal(ce, c_r, err_msg=tag)
    else:
        assert not np.any(ce & ~c_r), tag
    _note("certificate", len(ce))
    return ce, c_r


def test_certificate_cases_land_in_their_branches_on_the_device():
    n_cert = 0
    for name, (sdf, cen, eps, thres, cfg, want) in rc.certificate_cases().items():
        ce, c_r = _compare_certificates(sdf, cen, eps, thres, cfg, name)
        assert bool(ce[0]) == want.startswith("cert_"), (name, want)
        n_cert += int(ce[0])
    assert n_cert >= 15


@pytest.mark.parametrize("eps", rc.CERT_EPS_VALUES)
@pytest.mark.parametrize("H,W,cfg", [(40, 64, (2, 3, 1)), (23, 37, (2, 3, 2)), (16, 16, (0, 5, 0)), (40, 64, (0, 1, 1)), (160, 160, (10, 9, 3))])
def test_certificate_on_object_fields(H, W, cfg, eps):
    sdf, cen = rc.object_fields(2 if H * W == 25600 else 6, H, W, 21 + H)
    sdf, cen = torch.cat([sdf, sdf - 5.0]), torch.cat([cen, cen * 0.1])                 # with maps that have no peak
    _, mx_r, _ = rc.peak_pick(sdf, cen, *cfg)
    assert (mx_r > 0).any()
    bound = rc.cert_bound(eps)
    k = int(np.argmax(mx_r))
    n = 0
    for thres in (0.009, 0.05, mx_r[k] + 0.9 * bound, mx_r[k] + 1.1 * bound):
        ce, c_r = _compare_certificates(sdf, cen, eps, float(thres), cfg, f"{H}x{W} {cfg} eps {eps} thres {thres}")
        n += int(ce.sum())
    if cfg[0] >= 1 and eps <= 2e-4:
        assert n >= 4                                                                   # something was certified


def test_certificate_one_pixel_over_the_lds_limit_is_refused_before_any_launch():
    from unmore_amd import _lib as L, reasoning
    from unmore_amd.ops import _p, _stream
    H, W = 160, 161
    sdf, cen = torch.zeros(1, H, W, device="cuda"), torch.zeros(1, 2, H, W, device="cuda")
    mx, am, ce = _sentinels(1)
    st = L.lib().umr_center_peaks_certified(_p(sdf), _p(cen), _p(reasoning._anti_center_filter(sdf.device)), _p(mx), _p(am), _p(ce), 1, H, W,
                                            10, 9, 3, 2e-4, 0.009, _stream())
    with pytest.raises(RuntimeError, match="larger than the LDS mask planes"):
        L.check(st, "umr_center_peaks_certified")
    torch.cuda.synchronize()
    assert mx.item() == -7.5 and am.item() == -7 and ce.item() == -7


def test_certified_maps_keep_argmax_and_decision_under_perturbations_below_eps():
    """soundness by trial (40 x 64, (2, 3, 1)): 12 perturbations of max-norm 0.98 eps never move a certified map's argmax and never flip
    its `max > thres`, at the default threshold, a non-default one and one just outside the bound of a map's maximum"""
    from unmore_amd import reasoning
    eps, cfg = 2e-4, (2, 3, 1)
    sdf, cen = rc.object_fields(8, 40, 64, 31)
    extra = [rc.certificate_cases()[n] for n in ("peak_eps0.0002_thres0.009", "empty_neg_eps0.0002_thres0.009")]
    sdf = torch.cat([sdf, sdf - 5.0] + [e[0] for e in extra]).cuda()
    cen = torch.cat([cen, cen * 0.1] + [e[1] for e in extra]).cuda()
    _, mx_r, _ = rc.peak_pick(sdf, cen, *cfg)
    near = float(np.sort(mx_r[mx_r > 0])[len(mx_r[mx_r > 0]) // 2] + 1.1 * rc.cert_bound(eps))
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = 0.98 * eps
    total = 0
    for thres in (0.009, 0.05, near):
        mx, am, ce = reasoning.center_peaks_certified(sdf, cen, eps, singular_threshold=thres, **_cfg(cfg))
        assert int(ce.sum()) >= 4, ce.tolist()
        total += int(ce.sum())
        for t in range(12):
            if t % 3 == 0:
                ds = (torch.rand(sdf.shape, device="cuda", generator=gen) * 2 - 1) * a
                dc = (torch.rand(cen.shape, device="cuda", generator=gen) * 2 - 1) * a / 2 ** 0.5
            elif t % 3 == 1:
                ds = torch.sign(torch.rand(sdf.shape, device="cuda", generator=gen) - 0.5) * a
                dc = torch.sign(torch.rand(cen.shape, device="cuda", generator=gen) - 0.5) * a / 2 ** 0.5
            else:
                ramp = torch.linspace(-1, 1, sdf.shape[-1], device="cuda")
                ds = (ramp * (1 if t % 2 else -1)).expand_as(sdf) * a
                dc = (ramp.flip(0)).expand_as(cen) * a / 2 ** 0.5
            mx2, am2 = reasoning.center_peaks(sdf + ds, cen + dc, **_cfg(cfg))
            moved = ((am2 != am) | ((mx2 > thres) != (mx > thres))) & ce
            assert not bool(moved.any()), (thres, t, torch.nonzero(moved).flatten().tolist())
    _note("certificate soundness", 36)
    print(f"[reasoning kernels] certificate soundness: 3 thresholds x 12 perturbations, {total} certified maps, none moved")
    _line("certificate")


# ------------------------------------------------------------------------------------------------------------------ boundary deltas
@pytest.mark.parametrize("H,W", rc.DELTA_SHAPES)
def test_boundary_deltas_lie_in_the_derived_interval(H, W):
    from unmore_amd import reasoning
    for name, sdf in rc.delta_inputs(H, W).items():
        ref, lo, hi = rc.boundary_delta_intervals(sdf)
        out = torch.stack(reasoning.update_bbox_with_boundary_fields(sdf.cuda()), 1).cpu().double().numpy()
        err, half = np.abs(out - ref), np.maximum(hi - ref, ref - lo)
        i = np.unravel_index(np.argmax(np.where(half > 0, err / np.where(half > 0, half, 1), 0)), err.shape)
        print(f"[reasoning kernels] boundary_deltas {H}x{W} {name}: largest error {err[i]:.3e} of |delta| {abs(ref[i]):.3e}, interval half width "
              f"{half[i]:.3e}")
        _note("boundary_deltas", sdf.shape[0], 0, float(err[i]), float(half[i]))
        assert np.all((lo <= out) & (out <= hi)), (name, out, lo, hi)
    if (H, W) == rc.DELTA_SHAPES[-1]:
        _line("boundary_deltas")


# ------------------------------------------------------------------------------------------------------------------ components
def _components_on_device(mask, maxc, via_center=False):
    from unmore_amd import reasoning
    sdf, cen = rc.mask_to_fields(mask, via_center)
    counts, boxes = reasoning.mask_components(sdf.cuda(), cen.cuda(), max_components=maxc)
    return int(counts.item()), boxes[0].cpu().numpy()


@pytest.mark.parametrize("S", [1, 3, 15, 16, 33])
def test_mask_components_at_small_sides(S):
    for via in (False, True):                            # either half of the union switches the pixels on
        for name, m in rc.component_masks(S).items():
            n_r, b_r = rc.components(m)
            maxc = max(n_r, 1) + 3
            n, b = _components_on_device(m, maxc, via)
            assert n == n_r, (S, name, via)
            np.testing.assert_array_equal(b[:n_r], b_r, err_msg=f"{S} {name}")
            assert not b[n_r:].any()                                                    # zeros beyond the count
            _note("mask_components")
    if S == 33:
        _line("mask_components")


@pytest.mark.parametrize("S", [3, 15, 16, 33])
def test_mask_components_truncated_at_max_components(S):
    """more components than max_components: the TRUE count, the first max_components boxes, and nothing written past them"""
    from unmore_amd import _lib as L
    from unmore_amd.ops import _p, _stream
    m = rc.component_masks(S)["isolated"]
    n_r, b_r = rc.components(m)
    assert n_r >= 4
    sdf, cen = rc.mask_to_fields(m)
    sdf, cen = sdf.cuda(), cen.cuda()
    for maxc in (n_r - 1, n_r, n_r + 1, 1):
        counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        boxes = torch.full((maxc + 8, 4), -7, dtype=torch.int32, device="cuda")         # 8 guard rows behind the kernel's [maxc, 4]
        L.check(L.lib().umr_mask_components(_p(sdf), _p(cen), 1, S, maxc, _p(counts), _p(boxes), _stream()), "umr_mask_components")
        b = boxes.cpu().numpy()
        assert counts.item() == n_r
        k = min(maxc, n_r)
        np.testing.assert_array_equal(b[:k], b_r[:k])
        assert not b[k:maxc].any() and np.all(b[maxc:] == -7), (S, maxc)
        _note("mask_components truncated")


def test_mask_components_over_the_lds_budget_is_refused_before_any_launch():
    from unmore_amd import _lib as L
    from unmore_amd.ops import _p, _stream
    S = 128
    maxc = (150 * 1024 - S * S * 8) // 16 + 1
    assert S * S * 8 + maxc * 16 > 150 * 1024 >= S * S * 8 + (maxc - 1) * 16
    sdf, cen = torch.ones(1, S, S, device="cuda"), torch.zeros(1, 2, S, S, device="cuda")
    counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    boxes = torch.full((maxc, 4), -7, dtype=torch.int32, device="cuda")
    st = L.lib().umr_mask_components(_p(sdf), _p(cen), 1, S, maxc, _p(counts), _p(boxes), _stream())
    with pytest.raises(RuntimeError, match="exceed 150 KiB"):
        L.check(st, "umr_mask_components")
    torch.cuda.synchronize()
    assert counts.item() == -7 and bool((boxes == -7).all())


# ------------------------------------------------------------------------------------------------------------------ crop + resize
@pytest.mark.parametrize("S", [1, 7, 128])
def test_crop_resize_against_the_float32_restatement(S):
    """4 float32 ulp of the largest tap per output pixel (the blend's contracted forms); wherever no step of the blend rounds -- most ramp
    outputs: the source coordinate is exactly representable -- the device must return the restatement's bits, on the ramps the clamped
    source coordinate itself."""
    from unmore_amd import reasoning
    H, W = 20, 28
    boxes = rc.crop_boxes(H, W)
    g = torch.Generator().manual_seed(4)
    n_exact = 0
    for kind, img in (("random", torch.rand(3, H, W, generator=g).numpy() * 2 - 1), ("ramps", rc.ramp_images(H, W))):
        ref, big, SY, SX, exact = rc.crop_resize(img, boxes, S, with_taps=True)
        out, _ = reasoning.crop_resize(torch.from_numpy(img).cuda(), torch.tensor(boxes, dtype=torch.float64), S)
        out = out.cpu().numpy()
        err, tol = np.abs(out.astype(np.float64) - ref), 4 * np.spacing(big).astype(np.float64)
        i = np.unravel_index(np.argmax(err if err.any() else tol), err.shape)
        _note("crop_resize", len(boxes), 0, float(err[i]), float(tol[i]))
        assert np.all(err <= tol), (kind, S, i, float(err[i]), float(tol[i]))
        assert not out[-1].any()                                                        # the empty box
        np.testing.assert_array_equal(out[exact], ref[exact])                           # no step rounds there: no contraction can differ
        if kind == "ramps":
            for n, (x1, y1, x2, y2) in enumerate(boxes[:-1]):
                ex = np.broadcast_to((x1 + SX[n].astype(np.float64))[None, :], (S, S))
                ey = np.broadcast_to((y1 + SY[n].astype(np.float64))[:, None], (S, S))
                for ch, e in ((0, ex), (1, ey)):
                    n_exact += int(exact[n, ch].sum())
                    np.testing.assert_array_equal(out[n, ch][exact[n, ch]].astype(np.float64), e[exact[n, ch]])
    assert n_exact >= S * S
    print(f"[reasoning kernels] crop_resize S={S}: {n_exact} ramp outputs required exact")
    if S == 128:
        _line("crop_resize")
