"""Pins the restatements of tests/reasoning_common.py -- to the oracle at the one configuration the oracle knows, to hand-worked
cases, to scipy -- and proves that the constructed inputs of tests/test_reasoning_kernels_gpu.py do what they are for.  No GPU."""
import numpy as np
import pytest
import torch

import peaks_common as pc
import reasoning_common as rc
from oracle import objectness_oracle as orc
from unmore_amd import synth

EPS = 2e-4


def _fixture_fields(tag):
    if tag in pc.SYN:
        B, H, W, seed = pc.SYN[tag]
        return tuple(torch.from_numpy(a) for a in synth.object_like_fields(B, H, W, seed))
    g = pc.load()
    return torch.from_numpy(g[f"{tag}_sdf_maps"]), torch.from_numpy(g[f"{tag}_center_fields"])


TAGS = ["syn128", "syn96x160", "e2e_base128", "e2e_tiny128"]


@pytest.mark.parametrize("tag", TAGS)
def test_peak_pick_and_certificate_agree_with_the_oracle_at_its_configuration(tag):
    sdf, cen = _fixture_fields(tag)
    B = sdf.shape[0]
    # the fixture's maps plus the copies tests/test_certified_sweep_gpu.py uses for the other branches
    sdf_all, cen_all = torch.cat([sdf, sdf - 5.0, sdf]), torch.cat([cen, cen * 0.1, -cen])
    score_o, max_o, arg_o = orc.peak_pick(sdf_all, cen_all)
    score, mx, am = rc.peak_pick(sdf_all, cen_all, 10, 9, 3)
    assert (max_o > 0).any()
    np.testing.assert_array_equal(score != 0, score_o.numpy() != 0)                    # supports
    np.testing.assert_allclose(score, score_o.numpy(), atol=1e-12, rtol=0)
    np.testing.assert_array_equal(am, arg_o.numpy())
    np.testing.assert_allclose(mx, max_o.numpy(), atol=1e-12, rtol=0)
    for thres in (0.009, 0.05):
        a_o, p_o, c_o = orc.peak_certificate(sdf_all, cen_all, EPS, thres=thres, certify_empty=True)
        a, p, c, branch = rc.peak_certificate(sdf_all, cen_all, EPS, thres, 10, 9, 3, with_branch=True)
        np.testing.assert_array_equal(p, p_o.numpy())
        np.testing.assert_array_equal(c, c_o.numpy())                                  # the certified set
        np.testing.assert_allclose(a, a_o.numpy(), atol=1e-12, rtol=0)
    assert c[:B].sum() >= 1 and c[B:2 * B].sum() >= 1, branch                           # both certifying branches occur


@pytest.mark.parametrize("tag", TAGS)
def test_boundary_deltas_agree_with_the_oracle(tag):
    """The oracle forms the same float32 elementwise quantities and sums them in float32, in torch's order; the restatement sums in
    float64.  Whatever the order, a float32 sum of n non-negative terms is within (1 + u)^(n - 1) - 1 <= 1e-3 (n = 127 * 127) relative of
    the exact one: the oracle's deltas must lie in the interval the restatement derives for a summation depth of n - 1."""
    sdf, _ = _fixture_fields(tag)
    ref, lo, hi = rc.boundary_delta_intervals(sdf, depth=(sdf.shape[1] - 1) * (sdf.shape[2] - 1) - 1)
    out = torch.stack(orc.update_bbox_with_boundary_fields(sdf), 1).double().numpy()
    assert np.all((lo <= ref) & (ref <= hi))
    assert np.all((lo <= out) & (out <= hi)), np.abs(out - ref).max()
    assert np.all(hi - lo <= 4e-3 * np.abs(ref) + 1e-12)                               # the interval says something
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4)                         # (and the sides agree far better than it allows)


def test_crop_resize_agrees_with_the_oracle():
    g = torch.Generator().manual_seed(2)
    img = torch.rand(3, 48, 64, generator=g)
    boxes = [[0, 0, 64, 48], [3, 5, 40, 31], [30, 10, 34, 46], [60, 40, 64, 48], [5, 5, 9, 8], [7, 7, 8, 8]]
    for S in (1, 7, 128):
        ref = orc.crop_resize(img, boxes, S).numpy()
        out, big, _, _, _ = rc.crop_resize(img, boxes, S, with_taps=True)
        assert np.all(np.abs(out - ref) <= 4 * np.spacing(big)), (S, np.abs(out - ref).max())


def test_hand_worked_erosion():
    m = np.array([[1, 1, 1, 1, 1, 1, 0],
                  [1, 1, 1, 1, 1, 1, 0],
                  [1, 1, 1, 1, 1, 1, 0],
                  [1, 1, 1, 0, 1, 1, 0],
                  [1, 1, 1, 1, 1, 1, 0],
                  [1, 1, 1, 1, 1, 1, 1],
                  [1, 1, 1, 1, 1, 1, 1]], bool)
    # one round of 3 x 3: a pixel stays when all 9 of its window are set; the zero padding removes the rim
    one = np.array([[0, 0, 0, 0, 0, 0, 0],
                    [0, 1, 1, 1, 1, 0, 0],
                    [0, 1, 0, 0, 0, 0, 0],
                    [0, 1, 0, 0, 0, 0, 0],
                    [0, 1, 0, 0, 0, 0, 0],
                    [0, 1, 1, 1, 1, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0]], bool)
    np.testing.assert_array_equal(rc.erode(m, 3, 1), one)
    np.testing.assert_array_equal(rc.erode(m, 3, 2), np.zeros((7, 7), bool))           # no 3 x 3 block is left in `one`
    full = np.ones((7, 7), bool)
    two = np.zeros((7, 7), bool)
    two[2:5, 2:5] = True
    np.testing.assert_array_equal(rc.erode(full, 3, 2), two)                           # a full map loses one rim per round
    np.testing.assert_array_equal(rc.erode(full, 5, 1), two)
    np.testing.assert_array_equal(rc.erode(m, 1, 3), m)                                # k = 1 is the identity
    np.testing.assert_array_equal(rc.erode(m, 9, 0), m)                                # no round at all
    # against the oracle's float64 box convolution
    g = np.random.default_rng(0)
    r = g.random((3, 20, 31)) > 0.1
    for k, n in ((3, 1), (3, 2), (5, 1), (9, 3)):
        np.testing.assert_array_equal(rc.erode(r, k, n), orc.batch_erode(torch.from_numpy(r).long(), k, n).numpy() == 1)


def test_hand_worked_components():
    n, b = rc.components(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], bool))            # touching only diagonally: one component
    assert n == 1 and b.tolist() == [[0, 0, 2, 2]]
    ring = np.array([[0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 1, 1, 1, 1, 0],
                     [0, 1, 0, 0, 0, 1, 0],
                     [0, 1, 0, 1, 0, 1, 0],
                     [0, 1, 0, 0, 0, 1, 0],
                     [0, 1, 1, 1, 1, 1, 0],
                     [0, 0, 0, 0, 0, 0, 0]], bool)
    n, b = rc.components(ring)                                                          # the ring's first pixel comes before the dot's
    assert n == 2 and b.tolist() == [[1, 1, 6, 6], [3, 3, 4, 4]]
    n, b = rc.components(np.array([[0, 0, 1], [1, 0, 0]], bool))
    assert n == 2 and b.tolist() == [[2, 0, 3, 1], [0, 1, 1, 2]]
    assert rc.components(np.zeros((4, 4), bool))[0] == 0


@pytest.mark.parametrize("S", [1, 3, 15, 16, 33])
def test_components_agree_with_scipy_on_the_constructed_masks(S):
    from scipy import ndimage
    g = np.random.default_rng(S)
    masks = dict(rc.component_masks(S), random=g.random((S, S)) > 0.6)
    for name, m in masks.items():
        lab, n_ref = ndimage.label(m, structure=np.ones((3, 3)))
        ref = [[sl[1].start, sl[0].start, sl[1].stop, sl[0].stop] for sl in ndimage.find_objects(lab)]
        n, b = rc.components(m)
        assert n == n_ref and b.tolist() == ref, (S, name)
    # what the masks are for
    assert rc.components(masks["full"])[0] == 1 and rc.components(masks["diag_down"])[0] == 1 and rc.components(masks["diag_up"])[0] == 1
    assert rc.components(masks["serpentine"])[0] == 1 and masks["serpentine"].sum() >= S * S // 2
    assert rc.components(masks["rings"])[0] == (S + 3) // 4
    assert rc.components(masks["isolated"])[0] == ((S + 1) // 2) ** 2
    for via in (False, True):                                                           # both halves of the union build the mask
        for name, m in masks.items():
            np.testing.assert_array_equal(rc.union_mask(*rc.mask_to_fields(m, via_center=via))[0], m)


# ------------------------------------------------------------------------------------------------------------ vacuity guards
def test_peak_cases_have_peaks_where_intended_and_no_near_tie():
    n_maps = n_pos = 0
    for (H, W, cfg) in rc.PEAK_CASES:
        sdf, cen = rc.peak_case_fields(H, W)
        score, mx, am, bound = rc.peak_pick(sdf, cen, *cfg, with_bound=True)
        n_maps += len(mx)
        n_pos += int((mx > 0).sum())
        if (H, W, cfg) in rc.POSITIVE_PEAK_CASES:
            assert mx[0] > 0, (H, W, cfg)                                               # the converging map has a positive peak
        border = cfg[0]
        if min(H, W) <= 2 * border:                                                     # too small for the configuration
            assert np.all(mx == 0.0) and np.all(am == 0) and not score.any(), (H, W, cfg)
        for b in range(len(mx)):                                                        # no near-tie on the chosen seeds
            if mx[b] != 0.0:
                flat, bd = score[b].reshape(-1).copy(), bound[b].reshape(-1)
                flat[am[b]] = -np.inf
                second = int(flat.argmax())
                assert mx[b] - flat[second] > 2 * (bd[am[b]] + bd[second]), (H, W, cfg, b)
    assert len(rc.POSITIVE_PEAK_CASES) >= 13 and n_pos >= n_maps // 3
    assert (240, 320, (10, 9, 3)) in rc.POSITIVE_PEAK_CASES


def test_score_bound_is_tighter_than_the_suites_1e12():
    sdf, cen = rc.peak_case_fields(40, 64)
    score, _, _, bound = rc.peak_pick(sdf, cen, 0, 5, 0, with_bound=True)
    assert 0 < bound.max() < 1e-14
    # and it can fail: float32 accumulation of the same taps is far outside it
    c = cen.numpy()
    f = rc.anti_center_filter().astype(np.float32)
    p = np.zeros((c.shape[0], 2, 44, 68), np.float32)
    p[:, :, 2:42, 2:66] = c
    acc = np.zeros((c.shape[0], 40, 64), np.float32)
    for ch in range(2):
        for fi in range(5):
            for fj in range(5):
                acc += p[:, ch, fi:fi + 40, fj:fj + 64] * f[ch, fi, fj]
    live = score != 0
    assert (np.abs(acc / np.float32(24) - score)[live] > bound[live]).mean() > 0.9


@pytest.mark.parametrize("name", list(rc.TIE_CASES))
def test_tie_cases_have_two_bit_equal_maxima_at_the_intended_indices(name):
    sdf, cen, i1, i2 = rc.tie_fields(name)
    score, mx, am = rc.peak_pick(sdf, cen, *rc.TIE_CONFIG)
    flat = score.reshape(-1)
    assert i1 < i2 and flat[i1] == flat[i2] == mx[0] > 0 and am[0] == i1
    assert (flat == mx[0]).sum() == 2
    if name == "cross":
        assert i2 % 256 < i1 % 256          # the later pixel sits in the lower thread: the reduction must compare indices
    else:
        assert i2 % 256 == i1 % 256         # one thread owns both: its strided loop must keep the first
    H, W = sdf.shape[1:]
    for i in (i1, i2):                      # no tap skipped, not in the border
        y, x = divmod(i, W)
        assert 2 + 5 <= y < H - 7 and 2 + 5 <= x < W - 7
    _, _, cert, branch = rc.peak_certificate(sdf, cen, EPS, 0.009, *rc.TIE_CONFIG, with_branch=True)
    assert not cert[0] and branch == ["unc_runner"]


def test_all_negative_map():
    sdf, cen = rc.diverging_full_mask()
    assert sdf.shape[1] * sdf.shape[2] < 256
    score, mx, am = rc.peak_pick(sdf, cen, 0, 5, 0)
    assert (score < 0).all() and mx[0] < 0 and am[0] != 0 and mx[0] == score.max()
    assert (np.sort(score.reshape(-1))[-1] - np.sort(score.reshape(-1))[-2]) > 1e-6
    score, mx, am = rc.peak_pick(sdf, cen, 2, 5, 0)
    assert not score.any() and mx[0] == 0.0 and am[0] == 0


def test_certificate_cases_land_in_their_branches():
    cases = rc.certificate_cases()
    seen = set()
    for name, (sdf, cen, eps, thres, cfg, want) in cases.items():
        mx, am, cert, branch = rc.peak_certificate(sdf, cen, eps, thres, *cfg, with_branch=True)
        assert branch == [want], (name, branch, float(mx[0]))
        assert bool(cert[0]) == want.startswith("cert_")
        seen.add((want, eps))
        bound = rc.cert_bound(eps)
        if name.startswith("thres_inside"):
            assert 0 < thres - mx[0] < bound
        if name.startswith("thres_outside"):
            assert bound < thres - mx[0] < 1.2 * bound
        if name.startswith("empty_small_thres"):
            assert 0 < abs(thres) < bound and mx[0] == 0.0
    for eps in rc.CERT_EPS_VALUES:
        for want in ("cert_peak", "unc_runner", "cert_empty", "unc_empty"):
            assert (want, eps) in seen, (want, eps)
    for eps in rc.CERT_EPS_VALUES[1:]:
        assert ("unc_thres", eps) in seen and ("unc_min_mask", eps) in seen


def test_certificate_hw1_clause_and_border0_runner():
    """HW == 1: no other pixel, no zero outside: the runner-up clause is empty.  border == 0 and a full largest mask with every other
    score negative: the restatement's runner-up is that negative score (the kernel clamps it to 0: stricter, see the GPU test)."""
    sdf, cen = rc.diverging_full_mask()
    c = -cen                                            # converging on a 3 x 4 map: positive scores
    mx, am, cert, branch = rc.peak_certificate(sdf, c, 0.0, 0.5, 0, 5, 0, with_branch=True)
    assert mx[0] > 0 and branch[0] in ("cert_peak", "unc_runner")


def test_boundary_interval_is_derived_not_loose():
    sdf, _ = rc.object_fields(3, 128, 128, 1)
    ref, lo, hi = rc.boundary_delta_intervals(sdf)
    assert np.all((lo <= ref) & (ref <= hi))
    assert np.all(hi - lo < 2 * (1e-4 + 1e-4 * np.abs(ref)))          # inside the older test's atol + rtol
    rel = (hi - lo) / 2 / np.abs(ref)
    print(f"boundary deltas 128x128: half width / |delta| max {rel.max():.2e}")
    assert rel.max() < 5e-5
    # a float32 sum in an unfavourable order (one long chain) of the SAME terms is what the bound must tell apart at scale: the chain's
    # depth is n, not ceil(n / 256) + 8 -- its interval is wider
    _, lo2, hi2 = rc.boundary_delta_intervals(sdf, depth=127 * 127)
    assert np.all(hi2 - lo2 > 10 * (hi - lo))


def test_crop_ramp_outputs_are_the_source_coordinates():
    H, W = 20, 28
    img = rc.ramp_images(H, W)
    boxes = rc.crop_boxes(H, W)
    for S in (1, 7, 128):
        out, _, SY, SX, exact = rc.crop_resize(img, boxes, S, with_taps=True)
        assert exact[:-1, :2].mean() > 0.5                  # most ramp outputs involve no rounding at all: required bit-exact on the device
        for n, (x1, y1, x2, y2) in enumerate(boxes):
            if x2 <= x1 or y2 <= y1:
                assert not out[n].any()
                continue
            # channel 0 is the x ramp, channel 1 the y ramp: blend of a and a + 1 with weights 1 - l, l = the coordinate itself
            ex = (x1 + SX[n].astype(np.float64))[None, :].repeat(S, 0)
            ey = (y1 + SY[n].astype(np.float64))[:, None].repeat(S, 1)
            assert np.abs(out[n, 0] - ex).max() <= 4 * np.spacing(np.float32(W)) and np.abs(out[n, 1] - ey).max() <= 4 * np.spacing(np.float32(H))
            assert np.all(out[n, 0][exact[n, 0]] == ex[exact[n, 0]]) and np.all(out[n, 1][exact[n, 1]] == ey[exact[n, 1]])


@pytest.mark.parametrize("H,W", rc.DELTA_SHAPES)
def test_boundary_inputs_are_what_they_are_for_and_their_intervals_say_something(H, W):
    inp = rc.delta_inputs(H, W)
    for name, sdf in inp.items():
        ref, lo, hi = rc.boundary_delta_intervals(sdf)
        assert np.all(np.isfinite(ref)) and np.all((lo <= ref) & (ref <= hi)), name
        assert np.all(hi - lo <= 2e-4 * np.abs(ref) + 1e-30), (name, ((hi - lo) / np.abs(ref)).max())
    v, nr, fg, bg = rc._delta_parts(inp["constant"])
    assert not nr.any()
    assert np.allclose(np.abs(rc.boundary_deltas(inp["constant"])[:2]), 1e10 * np.array([[0.7], [0.3]]), rtol=1e-6)
    v, nr, fg, bg = rc._delta_parts(inp["saturated"])
    assert (bg[v == 50] == 0).all() and (fg[v == 50] == 1).all() and (v == 50).any() and (v == -50).any()
    assert (rc._delta_parts(inp["negative"])[0] < 0).all()
