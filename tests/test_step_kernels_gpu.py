"""LayerNorm (csrc/norm.hip), the bilinear resize and its adjoint, the head output layer, the fused loss and Adam (csrc/elementwise.hip),
each called through its ops wrapper and compared with the float64 restatement of tests/step_kernels_common.py (itself checked against
F.layer_norm / F.interpolate / autograd / the oracle's loss in tests/test_step_kernels_cpu.py).

Two kinds of test:
 bounded: random inputs at small shapes; the reference is float64 on exactly the tensors the kernel is given; every element must obey
          |kernel - ref| <= bound, the bound being a function of step_kernels_common built from reference quantities only (its
          docstring has the derivations).  `worst error / bound` is printed for every kernel and type.
 exact:   launch plans, block loops, ragged tails, reductions over many blocks.  The inputs are small integers and dyadic fractions for
          which every f32 operation of the kernel is exact (test_step_kernels_cpu.py proves it), so the result must EQUAL float64.
          Every such test asserts through the launch-plan mirror that its shape reaches the plan it names.
No tolerance below is a number of this file."""
import functools

import pytest
import torch
import torch.nn.functional as F

import step_kernels_common as sk

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
EPS32 = float(torch.tensor(1e-6, dtype=torch.float32))        # what the kernel receives for eps = 1e-6
SENTINEL = 7680.0                                             # exact in bf16, outside every value range below


def _ops():
    from unmore_amd import ops
    return ops


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def _randn(shape, seed, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(dtype)


def _nan(shape):
    return torch.full(shape, float("nan"), device=DEV)


def _check(label, out, ref, delta):
    """every element of `out` within the bound that belongs to its type; prints worst error / bound"""
    ratio, bad = sk.worst_ratio(out, ref, sk.out_bound(ref, delta, out.dtype))
    print(f"worst error / bound  {label} [{_name(out.dtype)}]: {ratio:.4f}")
    assert bad == 0, f"{label}: {bad} of {out.numel()} elements over their bound, worst error / bound = {ratio:.3f}"
    return ratio


def _same(out, ref):
    """bit for bit what float64 gives, rounded once to the result's type (the exact tests' values need no rounding in f32)"""
    return torch.equal(out.double(), ref.to(out.dtype).double())


# ------------------------------------------------------------------------------------------------------------- LayerNorm, bounded
LN_D = [(8, "one active lane"), (64, "one full chunk of the bf16x8 kernels"), (264, "a partly filled chunk"), (384, "the small backbone"),
        (1024, "the last D of the <2> kernels"), (1032, "the first D of the <4> kernels, chunk 4 of the generic ones"), (2048, "the largest D")]
LN_M = (1, 2, 7, 9, 37)          # odd tails of the two-rows-per-wave forward, one and several workgroups


def _ln_case(M, D, dtype, seed):
    x = _randn((M, D), seed, dtype, 1.5, 0.3)
    return x, _randn((D,), seed + 1, scale=0.1, shift=1.0), _randn((D,), seed + 2, scale=0.1), _randn((M, D), seed + 3, dtype), _randn((M, D), seed + 4, dtype)


def _ln_bounded(x, g, b, dy, dres, tag):
    ops = _ops()
    M, D = x.shape
    y, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6)
    r = sk.ln_fwd(x, g, b, EPS32)
    _check(f"ln_fwd y {tag}", y, r["y"], r["dy"])
    _check(f"ln_fwd mean {tag}", mean, r["mean"], r["dmean"])
    _check(f"ln_fwd rstd {tag}", rstd, r["rstd"], r["drstd"])
    for res, acc in ((None, False), (dres, True)):
        prior = (_randn((D,), 91), _randn((D,), 92)) if acc else None
        dgm, dbt = (prior[0].clone(), prior[1].clone()) if acc else (_nan((D,)), _nan((D,)))
        dx = ops.layernorm_bwd(dy, x, g, mean, rstd, dgm, dbt, dres=res, accumulate=acc)
        w = sk.ln_bwd(dy, x, g, mean, rstd, dres=res, prior=prior)          # from the mean / rstd the kernel was handed
        kind = "dres+acc" if acc else "plain"
        _check(f"ln_bwd dx {kind} {tag}", dx, w["dx"], w["ddx"])
        _check(f"ln_bwd dgamma {kind} {tag}", dgm, w["dgamma"], w["ddgamma"])
        _check(f"ln_bwd dbeta {kind} {tag}", dbt, w["dbeta"], w["ddbeta"])
    return y, mean, rstd


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", [d for d, _ in LN_D])
def test_layernorm_bounded(D, dtype):
    for M in LN_M:
        _ln_bounded(*_ln_case(M, D, dtype, D * 100 + M), tag=f"M={M} D={D}")


@pytest.mark.parametrize("D", [8, 1032, 2048])
def test_layernorm_planes_equal_the_f32_path(D):
    ops = _ops()
    for M in LN_M:
        x, g, b, _, _ = _ln_case(M, D, torch.float32, D * 100 + M)
        y, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6)
        yp, mean_p, rstd_p = ops.layernorm_fwd(x, g, b, 1e-6, planes=True)
        assert yp.shape == (M, 3 * D) and torch.equal(ops.unsplit3(yp), y)
        assert torch.equal(mean_p, mean) and torch.equal(rstd_p, rstd)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layernorm_extreme_rows_bounded(dtype):
    """the rows of test_extremes_gpu.py -- mean 3e3 + unit noise, exactly constant rows, rows of magnitude 1e4 and 1e-4, zero rows --
    under the bound, no row masked out: a row of variance ~ 0 has rstd ~ eps^-1/2 and the bound says so through rstd"""
    D = 768
    rows = [_randn((8, D), 1, shift=3e3), torch.full((4, D), 7.25, device=DEV), _randn((8, D), 2, scale=1e4), _randn((8, D), 3, scale=1e-4),
            torch.zeros((2, D), device=DEV)]
    x = torch.cat(rows).to(dtype)
    g, b = _randn((D,), 4, scale=0.1, shift=1.0), _randn((D,), 5, scale=0.1)
    dy, dres = _randn(x.shape, 6, dtype), _randn(x.shape, 7, dtype)
    y, mean, rstd = _ln_bounded(x, g, b, dy, dres, tag="extreme rows")
    assert all(bool(torch.isfinite(t.float()).all()) for t in (y, mean, rstd))
    r = sk.ln_fwd(x, g, b, EPS32)
    const = slice(8, 12)
    assert bool((r["mean"][const] == 7.25).all()) and bool(((r["rstd"][const] - EPS32 ** -0.5).abs() <= 1e-9).all())
    assert bool(((mean[const].double() - 7.25).abs() <= r["dmean"][const]).all())
    assert bool(((rstd[const].double() - EPS32 ** -0.5).abs() <= r["drstd"][const]).all())
    assert bool((mean[-2:] == 0).all()) and bool(torch.isfinite(r["drstd"]).all())


# ------------------------------------------------------------------------------------------------------------- LayerNorm backward, exact
def _ln_exact_cases():
    cus = sk.device_cus()
    return [(8, "one workgroup, one slab"), (897, "113 slabs: phase 0 of the reduce pass takes its 8-deep loop"),
            (905, "114 slabs: phases 0 and 1 take the 8-deep loop"), (16 * cus + 333, "9 or 10 rows per workgroup, deep loop + tail"),
            (48 * cus + 5, "25 rows per workgroup, a last workgroup with fewer rows")]


def _ln_exact(M, D, dtype, with_dx):
    ops = _ops()
    i = sk.ln_exact_inputs(M, D, 1000 + M % 997, DEV)
    x, dy, dres = i["x"].to(dtype), i["dy"].to(dtype), i["dres"].to(dtype)
    for res, acc in ((None, False), (dres, True)):
        prior = i["prior"] if acc else None
        dgm, dbt = (prior[0].clone(), prior[1].clone()) if acc else (_nan((D,)), _nan((D,)))
        dx = ops.layernorm_bwd(dy, x, i["gamma"], i["mean"], i["rstd"], dgm, dbt, dres=res, accumulate=acc)
        w = sk.ln_bwd(dy, x, i["gamma"], i["mean"], i["rstd"], dres=res, prior=prior)
        assert torch.equal(dgm.double(), w["dgamma"]), f"dgamma M={M} D={D} acc={acc}: {int((dgm.double() != w['dgamma']).sum())} differ"
        assert torch.equal(dbt.double(), w["dbeta"]), f"dbeta M={M} D={D} acc={acc}: {int((dbt.double() != w['dbeta']).sum())} differ"
        if with_dx:
            assert _same(dx, w["dx"]), f"dx M={M} acc={acc}: {int((dx.double() != w['dx'].to(dtype).double()).sum())} differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", range(5))
def test_layernorm_backward_exact_over_many_slabs(case, dtype):
    cus = sk.device_cus()
    M, why = _ln_exact_cases()[case]
    nb, rpb = sk.ln_bwd_plan(M, cus)
    deep = [sk.ln_reduce_deep(nb, ph) for ph in range(16)]
    if case == 0:
        assert (nb, rpb) == (1, 8)
    elif case == 1:
        assert (nb, rpb) == (113, 8) and deep[0][0] == 1 and all(d[0] == 0 for d in deep[1:]), why
    elif case == 2:
        assert (nb, rpb) == (114, 8) and deep[0][0] == 1 and deep[1][0] == 1 and deep[2][0] == 0 and M - (nb - 1) * rpb == 1, why
    elif case == 3:
        assert rpb in (9, 10) and nb <= 2 * cus and deep[0][0] >= 1 and deep[0][1] >= 1, why
    else:
        assert rpb == 25 and 0 < M - (nb - 1) * rpb < rpb and deep[0][0] >= 1, why
    _ln_exact(M, 64, dtype, with_dx=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", [1032, 2048])
def test_layernorm_backward_parameter_sums_exact_at_wide_rows(D, dtype):
    """the <4> kernels and chunks 4..7 of the generic ones; 1 / D is not a power of two at 1032, so only dgamma / dbeta are exact"""
    assert sk.ln_bwd_plan(905, sk.device_cus()) == (114, 8)
    _ln_exact(905, D, dtype, with_dx=False)


# ------------------------------------------------------------------------------------------------------------- resize, bounded
# (B, Hi, Wi, C, Ho, Wo, align, the adjoint's kernel in bf16 or None, slice geometry or None for the default)
WIDE8 = (8, 40, 16, 24, 8, 8, 0, 16)       # x = wide[..., 8:8+C] of C+40; y into [16:16+C] of C+24; dy = [8:] of C+8; dx into [:C] of C+16
WIDE4 = (4, 12, 4, 8, 4, 4, 4, 8)          # offsets of 4 elements: pixel strides that are no multiple of 8 -> the NV = 1 kernels
RESIZE = (
    # tests/test_kernels_gpu.py::test_bilinear
    [(2, 6, 4, 16, 12, 8, True, None, None), (2, 12, 12, 16, 24, 24, True, None, None), (2, 24, 24, 16, 8, 8, False, None, None),
     (2, 24, 24, 16, 37, 30, False, None, None), (2, 19, 19, 16, 37, 37, True, None, None), (2, 1, 1, 16, 2, 2, True, None, None),
     (2, 48, 40, 16, 96, 80, True, None, None), (2, 25, 13, 16, 49, 26, True, None, None), (2, 48, 40, 16, 96, 80, False, None, None)]
    # tests/test_commute_gpu.py::test_row_stream_resizes_at_other_scales
    + [(B, Hi, Wi, C, Ho, Wo, a, None, None) for a in (True, False)
       for (B, Hi, Wi, C, Ho, Wo) in [(2, 24, 40, 32, 12, 20), (1, 1, 7, 16, 5, 14), (2, 37, 37, 64, 74, 74), (1, 30, 30, 24, 44, 52), (3, 5, 6, 8, 64, 3)]]
    # tests/test_commute_gpu.py::test_resize_on_column_slices_with_relu
    + [(2, 12, 20, 64, 24, 40, True, None, None), (1, 9, 9, 16, 23, 17, True, None, None), (3, 16, 16, 512, 32, 32, True, None, None)]
    # the thresholds of the adjoint's kernel choice: scale exactly 0.4 / 0.45 / 0.49, and x2 with align_corners where (Wi-1)/(2Wi-1) crosses 0.49
    + [(1, 3, Wi, C, 6, Wo, a, k, None) for C in (8, 24)
       for (Wi, Wo, a, k) in [(2, 5, False, "rowstream8"), (4, 10, False, "rowstream8"), (10, 21, True, "rowstream8"), (50, 101, True, "rowstream6"),
                              (25, 50, True, "rowstream8"), (26, 52, True, "rowstream6")]]
    # C = 4, 12 and slices at offsets of 4 elements: the generic NV = 1 kernels (in bf16 too)
    + [(2, 6, 5, 4, 12, 10, True, "generic1", WIDE4), (2, 7, 9, 12, 14, 18, False, "generic1", WIDE4), (1, 9, 9, 16, 18, 18, True, "generic1", WIDE4)]
    # an upscale of more than 2.5: the adjoint's generic fallback in bf16
    + [(1, 5, 7, 8, 14, 20, True, "generic2", None), (2, 4, 6, 16, 11, 17, False, "generic2", None)])
RESIZE_IDS = ["B%dx%dx%dxC%d-%dx%d-%s%s" % (s[:6] + ("align" if s[6] else "half", "-off4" if s[8] == WIDE4 else "")) for s in RESIZE]


def _resize_bounded(shape, dtype, tag):
    ops = _ops()
    B, Hi, Wi, C, Ho, Wo, align, kernel, geo = shape
    xo, xp, yo, yp, dyo, dyp, dxo, dxp = geo or WIDE8
    if kernel is not None and dtype == torch.bfloat16:          # the dense call without slice geometry, the slice-to-slice call with it
        ld = dict(lddy=C + dyp, lddx=C + dxp) if geo else {}
        assert sk.resize_bwd_plan(B, Hi, Wi, Ho, Wo, C, align, dtype, **ld)["kernel"] == kernel
        if geo:
            assert sk.resize_fwd_plan(B, Ho, Wo, C, dtype, ldx=C + xp, ldy=C + yp)["kernel"] == "generic1"
    seed = Hi * 1000 + Wo
    wide = _randn((B, Hi, Wi, C + xp), seed, dtype)
    xs = wide[..., xo:xo + C]
    x = xs.contiguous()
    ref, bound = sk.resize_fwd(x, Ho, Wo, align)
    worst = _check(f"resize fwd {tag}", ops.bilinear_fwd(x, Ho, Wo, align), ref, bound)
    y_slice_in = ops.bilinear_fwd(xs, Ho, Wo, align)
    assert y_slice_in.is_contiguous()
    _check(f"resize fwd from a slice {tag}", y_slice_in, ref, bound)
    owide = torch.full((B, Ho, Wo, C + yp), SENTINEL, dtype=dtype, device=DEV)
    ops.bilinear_fwd(xs, Ho, Wo, align, relu=True, out=owide[..., yo:yo + C])
    _check(f"resize fwd relu into a slice {tag}", owide[..., yo:yo + C], ref.clamp_min(0), bound)
    assert bool((owide[..., :yo] == SENTINEL).all()) and bool((owide[..., yo + C:] == SENTINEL).all())
    _check(f"resize fwd relu {tag}", ops.bilinear_fwd(x, Ho, Wo, align, relu=True), ref.clamp_min(0), bound)
    # the adjoint, dense and slice to slice
    dyw = _randn((B, Ho, Wo, C + dyp), seed + 1, dtype)
    dys = dyw[..., dyo:dyo + C]
    dy = dys.contiguous()
    ref, bound = sk.resize_bwd(dy, Hi, Wi, align)
    worst = max(worst, _check(f"resize bwd {tag}", ops.bilinear_bwd(dy, Hi, Wi, align), ref, bound))
    dxw = torch.full((B, Hi, Wi, C + dxp), SENTINEL, dtype=dtype, device=DEV)
    ops.bilinear_bwd(dys, Hi, Wi, align, out=dxw[..., dxo:dxo + C])
    _check(f"resize bwd slice to slice {tag}", dxw[..., dxo:dxo + C], ref, bound)
    assert bool((dxw[..., :dxo] == SENTINEL).all()) and bool((dxw[..., dxo + C:] == SENTINEL).all())
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", RESIZE, ids=RESIZE_IDS)
def test_resize_bounded(shape, dtype):
    _resize_bounded(shape, dtype, RESIZE_IDS[RESIZE.index(shape)])


X2 = [(2, 12, 12, 16, 24, 24, True), (2, 37, 37, 64, 74, 74, False), (4, 3, 26, 24, 6, 52, True), (2, 48, 40, 16, 96, 80, True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("shape", X2, ids=["12x12", "37x37xC64", "3x26", "48x40"])
def test_resize_with_capped_grid_rows_equals_the_uncapped_call(shape, cap, dtype, umr_opts):
    """UMR_BILINEAR_GY = 1 / 3: every block loops over several rows (generic kernels) or runs (row-stream kernels)"""
    ops = _ops()
    B, Hi, Wi, C, Ho, Wo, align = shape
    for plan in (sk.resize_fwd_plan(B, Ho, Wo, C, dtype, gy_cap=cap), sk.resize_bwd_plan(B, Hi, Wi, Ho, Wo, C, align, dtype, gy_cap=cap)):
        assert plan["gy"] == cap and plan["units"] >= 2 * cap + 1, plan           # at least two full rounds and a ragged one
    x, dy = _randn((B, Hi, Wi, C), 5, dtype), _randn((B, Ho, Wo, C), 6, dtype)
    umr_opts.delenv("UMR_BILINEAR_GY", raising=False)
    y0, dx0 = ops.bilinear_fwd(x, Ho, Wo, align), ops.bilinear_bwd(dy, Hi, Wi, align)
    umr_opts.setenv("UMR_BILINEAR_GY", str(cap))
    y1, dx1 = ops.bilinear_fwd(x, Ho, Wo, align), ops.bilinear_bwd(dy, Hi, Wi, align)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    _check(f"resize fwd GY={cap} {shape}", y1, *sk.resize_fwd(x, Ho, Wo, align))
    _check(f"resize bwd GY={cap} {shape}", dx1, *sk.resize_bwd(dy, Hi, Wi, align))


# ------------------------------------------------------------------------------------------------------------- resize, long runs (bf16)
# the plans the engine uses on its feature maps: the rolling two-row state, the prefetch of row cury + 2 and the retire() chain over
# runs of 16 / 8 (forward) and 12 / 6 (adjoint) rows.  Smallest B that reaches each plan at C = 512 (22 / 11 column blocks):
LONG_FWD = [(32, 16, "32 * 3 runs * 22 column blocks = 2112 >= 2048"), (19, 8, "19 * 3 * 22 = 1254 < 2048 <= 19 * 5 * 22 = 2090")]
LONG_BWD = [(63, 12, "63 * 3 runs * 11 column blocks = 2079 >= 2048"), (38, 6, "38 * 3 * 11 = 1254 < 2048 <= 38 * 5 * 11 = 2090")]
CHUNK = 8                                  # images per reference evaluation: the float64 intermediates stay below 1 GB


def _interp64(x, Ho, Wo, dy=None):
    """F.interpolate in float64 (align_corners false); with dy its adjoint through autograd.  NHWC in and out."""
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(dy is not None)
    y = F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=False)
    if dy is None:
        return y.permute(0, 2, 3, 1)
    return torch.autograd.grad(y, xr, dy.double().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)


@pytest.mark.parametrize("align", [True, False], ids=["align-bounded", "half-exact"])
@pytest.mark.parametrize("B,run,why", LONG_FWD, ids=["run16", "run8"])
def test_resize_forward_long_runs(B, run, why, align):
    ops = _ops()
    Hi, Wi, C, Ho, Wo = 20, 43, 512, 40, 86
    plan = sk.resize_fwd_plan(B, Ho, Wo, C, torch.bfloat16)
    assert (plan["kernel"], plan["run"], plan["gx"]) == ("rowstream", run, 22) and (Ho % run != 0) == (run == 16), (plan, why)   # 16 + 16 + 8 rows
    x = (_randn((B, Hi, Wi, C), 1, torch.bfloat16) if align else sk.ints((B, Hi, Wi, C), 7, 1, DEV).bfloat16())
    y = ops.bilinear_fwd(x, Ho, Wo, align)
    worst = 0.0
    for b0 in range(0, B, CHUNK):
        xs, ys = x[b0:b0 + CHUNK], y[b0:b0 + CHUNK]
        if align:
            ref, bound = sk.resize_fwd(xs, Ho, Wo, True)
            ratio, bad = sk.worst_ratio(ys, ref, sk.out_bound(ref, bound, ys.dtype))
            assert bad == 0, (b0, bad, ratio)
            worst = max(worst, ratio)
        else:
            ref = _interp64(xs, Ho, Wo)
            assert torch.equal(ys.double(), ref), f"images {b0}..: {int((ys.double() != ref).sum())} elements differ"
        del ref
    if align:
        print(f"worst error / bound  resize fwd RUN={run} [bf16]: {worst:.4f}")


@pytest.mark.parametrize("align", [True, False], ids=["align-bounded", "half-exact"])
@pytest.mark.parametrize("B,run,why", LONG_BWD, ids=["run12", "run6"])
def test_resize_adjoint_long_runs(B, run, why, align):
    ops = _ops()
    Hi, Wi, C, Ho, Wo = 30, 43, 512, 60, 86
    plan = sk.resize_bwd_plan(B, Hi, Wi, Ho, Wo, C, align, torch.bfloat16)
    assert (plan["kernel"], plan["run"], plan["gx"]) == ("rowstream6" if align else "rowstream8", run, 11) and (Hi % run != 0) == (run == 12), (plan, why)   # 12 + 12 + 6 rows
    dy = (_randn((B, Ho, Wo, C), 2, torch.bfloat16) if align else sk.ints((B, Ho, Wo, C), 3, 2, DEV).bfloat16())
    dx = ops.bilinear_bwd(dy, Hi, Wi, align)
    worst = 0.0
    for b0 in range(0, B, CHUNK):
        ds, xs = dy[b0:b0 + CHUNK], dx[b0:b0 + CHUNK]
        if align:
            ref, bound = sk.resize_bwd(ds, Hi, Wi, True)
            ratio, bad = sk.worst_ratio(xs, ref, sk.out_bound(ref, bound, xs.dtype))
            assert bad == 0, (b0, bad, ratio)
            worst = max(worst, ratio)
        else:
            ref = _interp64(torch.zeros((ds.shape[0], Hi, Wi, C), device=DEV), Ho, Wo, dy=ds)
            assert torch.equal(xs.double(), ref), f"images {b0}..: {int((xs.double() != ref).sum())} elements differ"
        del ref
    if align:
        print(f"worst error / bound  resize bwd RUN={run} [bf16]: {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------- head output layer
HEAD_M = [(2, 9, 7), (3, 37, 41)]          # 126 rows: one block; 4551 rows: 18 blocks, ragged 64-row runs, runs that straddle an image
ACTS = [(sk.ACT_NONE, "none"), (sk.ACT_TANH, "tanh"), (sk.ACT_SINE, "sine")]


def _head_bounded(B, H, W, K, Cout, act, relu_mask, dtype, tag):
    ops = _ops()
    M = B * H * W
    h = _randn((M, K), K + M, dtype)
    w, bias = _randn((Cout, K), 2, scale=K ** -0.5), _randn((Cout,), 3)
    dout = _randn((B, Cout, H, W), 4)
    out = ops.head_out_fwd(h, w, bias, B, H, W, act)
    ref, bound, _ = sk.head_fwd(h, w, bias, B, H, W, act)
    _check(f"head fwd {tag}", out, ref, bound)
    # what the backward reads: tanh -> the saved output, sine -> the saved pre-activation (the kernel's own, act none)
    saved = out if act == sk.ACT_TANH else (ops.head_out_fwd(h, w, bias, B, H, W, sk.ACT_NONE) if act == sk.ACT_SINE else None)
    dw, db = _nan((Cout, K)), _nan((Cout,))
    dh = ops.head_out_bwd(h, w, dout, saved, act, relu_mask, dw, db)
    r = sk.head_bwd(h, w, dout, saved, act, relu_mask)
    _check(f"head bwd dh {tag}", dh, r["dh"], r["ddh"])
    _check(f"head bwd dw {tag}", dw, r["dw"], r["ddw"])
    _check(f"head bwd db {tag}", db, r["db"], r["ddb"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", HEAD_M, ids=["M126", "M4551"])
@pytest.mark.parametrize("K", [4, 64, 256, 1000, 1024])
def test_head_out_bounded(K, B, H, W, dtype, umr_opts):
    """K < 1024: threads without columns (the generic kernel's kok guard is false for some); K = 1024 in bf16: the k1024 kernel and,
    through UMR_HEAD_OUT_BWD_GENERIC, the generic one"""
    forms = ("k1024", "generic") if (K == 1024 and dtype == torch.bfloat16) else ("generic",)
    for form in forms:
        if form == "generic" and len(forms) == 2:
            umr_opts.setenv("UMR_HEAD_OUT_BWD_GENERIC", "1")
        else:
            umr_opts.delenv("UMR_HEAD_OUT_BWD_GENERIC", raising=False)
        for Cout in (1, 2):
            for act, an in ACTS:
                for relu_mask in (False, True):
                    _head_bounded(B, H, W, K, Cout, act, relu_mask, dtype, f"{form} K={K} M={B * H * W} Cout={Cout} {an} relu={int(relu_mask)}")


# (B, H, W, K, dtypes, (blocks, rows per block), why)
HEAD_EXACT = [
    (1, 257, 257, 8, DTYPES, (259, 256), "M > 65536: the forward's waves stride; 259 blocks of 256 rows, the last with 1"),
    (5, 1, 104873, 8, DTYPES, (2041, 257), "M = 524288 + 77: the 2048-block cap, 257 rows per block"),
    (3, 37, 41, 1024, [torch.bfloat16], (18, 253), "the k1024 kernel: ragged 64-row runs, runs that straddle an image"),
]


@pytest.mark.parametrize("Cout", [1, 2])
@pytest.mark.parametrize("case", range(len(HEAD_EXACT)), ids=["M66049", "M524365", "k1024"])
def test_head_out_exact_over_many_blocks(case, Cout, umr_opts):
    ops = _ops()
    B, H, W, K, dtypes, plan, why = HEAD_EXACT[case]
    M = B * H * W
    assert sk.head_out_blocks(M) == plan, (sk.head_out_blocks(M), why)
    if case == 0:
        assert sk.head_fwd_grid(M) == (16384, 2) and sk.head_fwd_grid(65536)[1] == 1
    umr_opts.delenv("UMR_HEAD_OUT_BWD_GENERIC", raising=False)
    h32, w, bias = sk.ints((M, K), 3, 1, DEV), sk.ints((Cout, K), 2, 2, DEV), sk.ints((Cout,), 2, 3, DEV)
    dout = sk.ints((B, Cout, H, W), 2, 4, DEV)
    for dtype in dtypes:
        h = h32.to(dtype)
        out = ops.head_out_fwd(h, w, bias, B, H, W, sk.ACT_NONE)
        assert torch.equal(out.double(), sk.head_fwd(h, w, bias, B, H, W, sk.ACT_NONE)[0]), f"forward {_name(dtype)}"
        for relu_mask in (False, True):
            dw, db = _nan((Cout, K)), _nan((Cout,))
            dh = ops.head_out_bwd(h, w, dout, None, sk.ACT_NONE, relu_mask, dw, db)
            r = sk.head_bwd(h, w, dout, None, sk.ACT_NONE, relu_mask)
            assert float(r["dw"].abs().max()) < 2 ** 24
            assert torch.equal(dw.double(), r["dw"]), f"dw {_name(dtype)}: {int((dw.double() != r['dw']).sum())} differ"
            assert torch.equal(db.double(), r["db"]), f"db {_name(dtype)}"
            assert _same(dh, r["dh"]), f"dh {_name(dtype)}"


# ------------------------------------------------------------------------------------------------------------- fused loss
def _loss_case(B, H, W, seed):
    pc, gc = _randn((B, 2, H, W), seed), _randn((B, 2, H, W), seed + 1)
    ps, gs = torch.tanh(_randn((B, 1, H, W), seed + 2)), torch.tanh(_randn((B, 1, H, W), seed + 3))
    sal = (_randn((B, 1, H, W), seed + 4) > 0).float()
    return pc, ps, gc, gs, sal


def _loss_bounded(B, H, W, switches, gscale, tag):
    ops = _ops()
    pc, ps, gc, gs, sal = _loss_case(B, H, W, B * 7 + H)
    out5, dpc, dps = ops.objectness_loss(pc, ps, gc, gs, sal, *switches, grad_scale=gscale)
    r = sk.loss(pc, ps, gc, gs, sal, *switches, gscale=gscale)
    _check(f"loss totals {tag}", out5, r["out5"], r["dout5"])
    _check(f"loss d_center {tag}", dpc, r["dpc"], r["ddpc"])
    _check(f"loss d_sdf {tag}", dps, r["dps"], r["ddps"])
    only, _, _ = ops.objectness_loss(pc, ps, gc, gs, sal, *switches, need_grad=False)
    assert torch.equal(only, ops.objectness_loss(pc, ps, gc, gs, sal, *switches)[0])          # the totals do not depend on the gradient outputs


SWITCHES = [(c, s, g, b) for c in (True, False) for s in (True, False) for g in (True, False) for b in (True, False)]


@pytest.mark.parametrize("center_l2,sdf_l2,use_grad,use_bce", SWITCHES)
@pytest.mark.parametrize("B,H,W", [(3, 11, 13), (2, 1, 9), (2, 9, 1)], ids=["3x11x13", "H1", "W1"])
def test_loss_bounded(B, H, W, center_l2, sdf_l2, use_grad, use_bce):
    """H = 1 / W = 1: the gradient-map term has no interior, its normaliser and its total are 0"""
    _loss_bounded(B, H, W, (center_l2, sdf_l2, use_grad, use_bce), 0.75, f"{B}x{H}x{W} {int(center_l2)}{int(sdf_l2)}{int(use_grad)}{int(use_bce)}")


@pytest.mark.parametrize("B,H,W,blocks", [(1, 11, 13, 1), (3, 11, 13, 2), (2, 160, 204, 255), (1, 256, 256, 256), (1, 257, 256, 257), (1, 512, 512, 1024)],
                         ids=["1", "2", "255", "256", "257", "1024"])
def test_loss_bounded_at_block_counts_around_the_tree(B, H, W, blocks):
    """loss_reduce_kernel: fewer partials than threads, exactly 256, one thread with two, all threads with four"""
    assert sk.loss_plan(B * H * W) == (blocks, 1)
    for switches in ((True, False, True, True), (False, True, True, False)):
        _loss_bounded(B, H, W, switches, 1.0, f"{blocks} blocks {switches}")


@pytest.mark.parametrize("l2", [True, False], ids=["l2", "l1"])
def test_loss_exact_with_two_grid_stride_iterations(l2):
    ops = _ops()
    B, H, W = 2, 512, 512
    assert sk.loss_plan(B * H * W) == (1024, 2)
    pc, ps, gc, gs = sk.loss_exact_inputs(B, H, W, 5, DEV)
    out5, dpc, dps = ops.objectness_loss(pc, ps, gc, gs, None, l2, l2, False, False, grad_scale=4.0)
    r = sk.loss(pc, ps, gc, gs, None, l2, l2, False, False, gscale=4.0)
    assert torch.equal(out5.double(), r["out5"]), (out5.double() - r["out5"])
    assert float(out5[3]) == 0 and float(out5[4]) == 0
    assert torch.equal(dpc.double(), r["dpc"]) and torch.equal(dps.double(), r["dps"])


# ------------------------------------------------------------------------------------------------------------- Adam
@functools.lru_cache(maxsize=None)
def _adam_problem():
    return [_randn((1000,), s) for s in (1, 2, 3, 4)]          # p0 and the gradients of three steps


@pytest.mark.parametrize("hyper", [False, True], ids=["scalars", "device-hyper"])
def test_adam_grid_stride_equals_the_small_problem_tiled(hyper):
    """n = 16384 * 256 + 13: the grid-stride loop runs twice for 13 threads.  The arrays tile a 1000-element problem, the per-element
    arithmetic is the same, so p, m and v must equal the tiled result of the 1000-element run (4 blocks, no loop)"""
    ops = _ops()
    n = 16384 * 256 + 13
    assert sk.adam_grid(n) == (16384, 2) and sk.adam_grid(1000) == (4, 1)
    p0, *grads = _adam_problem()
    idx = torch.arange(n, device=DEV) % 1000
    small = [p0.clone(), torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)]
    big = [p0[idx].contiguous(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    hy = torch.zeros(7, device=DEV)
    for step, g in enumerate(grads, start=1):
        gb = g[idx].contiguous()
        if hyper:
            ops.adam_set_hyper(hy, step, lr=1e-3)
            ops.adam_step_hyper(*small[:1], g, *small[1:], hy)
            ops.adam_step_hyper(*big[:1], gb, *big[1:], hy)
        else:
            ops.adam_step(small[0], g, small[1], small[2], step, lr=1e-3)
            ops.adam_step(big[0], gb, big[1], big[2], step, lr=1e-3)
    for name, s, b in zip("pmv", small, big):
        assert torch.equal(b, s[idx]), f"{name}: {int((b != s[idx]).sum())} elements differ"
    assert not torch.equal(small[0], p0)
