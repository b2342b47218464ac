"""Every umr_gemm_desc / umr_gemm_tn_desc form the engine launches, against the float64 restatement of gemm_forms_common.py: row
remaps on either side, broadcast aux rows, row strides longer than the row, outputs that alias their aux operand, aux2, the five
activations, one- and two-column outputs.  Remapped and strided inputs live inside NaN allocations (a wrong row shows as NaN and
stays in bounds), outputs inside sentinel allocations (what a call must not write is compared bit for bit).  The inventory test at
the end records the forms of a train step and of the classifier and fails on one that no kernel test pins."""
import pytest
import torch

import gemm_forms_common as C

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


@pytest.fixture
def f32_mode_restored():
    from unmore_amd import ops
    prev = ops.get_f32_mode()
    yield
    ops.set_f32_mode(prev)


def _modes(dtype, K):
    """f32 runs in both product modes where they are different kernels: with K % 32 != 0 the NT launcher sends both to the exact-f32
    one (csrc/gemm_nt.hip, gemm_nt_impl)"""
    if dtype != F32:
        return (None,)
    return ("x3", "exact") if K % 32 == 0 else ("x3",)


def _set_mode(mode):
    from unmore_amd import ops
    if mode:
        ops.set_f32_mode(mode)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


def _assert_rest_untouched(big, before, view=None, rows=None):
    """allocation `big` equals its copy `before` bit for bit, except in rows `rows` (all, if None) of its view `view`"""
    changed = _bits(big) != _bits(before)
    if view is not None:
        cv = changed.as_strided(view.shape, view.stride(), view.storage_offset())
        if rows is None:
            cv.fill_(False)
        else:
            cv[rows] = False
    assert not bool(changed.any()), f"{int(changed.sum())} elements written outside the addressed rows / columns"


def _close(x, ref, dtype):
    torch.testing.assert_close(x.double(), ref, **C.tol(dtype))


def _tuple(r):
    return r if isinstance(r, tuple) else (r,)


# ------------------------------------------------------------------------------------------------ NT A-row gather
_GATHER = [(c, dt) for c in C.GATHER_CASES for dt in ((F32, BF16) if c[-1] == 128 else (BF16,))]


@pytest.mark.parametrize("readout", [False, True], ids=["plain", "readout"])
@pytest.mark.parametrize("case,dtype", _GATHER, ids=[f"{'x'.join(map(str, c))}-{'f32' if d == F32 else 'bf16'}" for c, d in _GATHER])
def test_nt_a_row_gather(case, dtype, readout, umr_opts, f32_mode_restored):
    """The readout's token gather (a_remap = (g, Nt, off)): tiles that cross several image ends, g larger than a tile, an offset of 2;
    plain and as the readout launches it (per-image rowbias by LOGICAL row, GELU, pre-activation saved).  Against float64, and bit
    for bit against the same kernel on a compact copy of the gathered rows."""
    from unmore_amd import ops
    dev = _dev()
    B, g, Nt, off, N, K, tile = case
    args, kw, compact = C.build_gather(case, dtype, dev, readout)
    umr_opts.setenv("UMR_GEMM_TILE", str(tile))
    umr_opts.setenv("UMR_NT_SPLITK", "0")
    if tile == 256:
        assert ops.gemm_nt(compact, args[1], None, query_rowreduce=True), "the shape must run on the 256x256 kernels"
        umr_opts.setenv("UMR_NT256_PERSIST", "0")   # the compact call would otherwise go to the persistent kernel (csrc/gemm_nt256.hip)
    ckw = {k: v for k, v in kw.items() if k not in ("M", "a_remap")}
    bigs, views = zip(*[C.sentinel(B * g, N, dtype, dev) for _ in range(2 if readout else 1)])
    before = [b.clone() for b in bigs]
    outs = dict(zip(("out", "out2"), views))
    ref, ref2 = C.ref_gemm_nt(*args, **kw)
    for mode in _modes(dtype, K):
        _set_mode(mode)
        for b, b0 in zip(bigs, before):
            b.copy_(b0)
        ops.gemm_nt(*args, **kw, **outs)
        for b, b0, v in zip(bigs, before, views):
            _assert_rest_untouched(b, b0, v)
        _close(views[0], ref, dtype)
        if readout:
            _close(views[1], ref2, dtype)
        same = _tuple(ops.gemm_nt(compact, args[1], None, **ckw))
        for a, b in zip(views, same):
            assert _same_bits(a, b), (mode, "gathered and compact operands differ")


# ------------------------------------------------------------------------------------------------ NT C side
_PATCH = [(c, dt) for c in C.PATCH_CASES for dt in ((F32, BF16) if c[4] == 128 else (BF16,))]


def _force_split_k(ops, umr_opts, monkeypatch, force):
    """UMR_NT_SPLITK = force, and the library's split-K scratch handed to every launch: ops.gemm_nt itself passes it from K = 768 on
    only (ops._wants_splitk_ws), the cases here are shorter"""
    umr_opts.setenv("UMR_NT_SPLITK", force)
    monkeypatch.setattr(ops, "_wants_splitk_ws", lambda d: True)


def _c_side(ops, args, kw, big, dtype, K, rows, force=None):
    """run one C-side call per f32 mode on a fresh copy of the output allocation; float64 check + nothing else written"""
    before = big.clone()
    ref, _ = C.ref_gemm_nt(*args, **kw)
    for mode in _modes(dtype, K):
        _set_mode(mode)
        big.copy_(before)
        if force:
            assert 1 < ops.gemm_nt(*args, **kw, query_splits=True) <= int(force)
        r = ops.gemm_nt(*args, **kw)
        assert r.data_ptr() == kw["out"].data_ptr()
        _close(kw["out"], ref, dtype)
        _assert_rest_untouched(big, before, kw["out"], rows)
    big.copy_(before)


@pytest.mark.parametrize("case,dtype", _PATCH, ids=[f"{'x'.join(map(str, c))}-{'f32' if d == F32 else 'bf16'}" for c, d in _PATCH])
def test_nt_patch_embed_form(case, dtype, umr_opts, f32_mode_restored, monkeypatch):
    """out = tokens [B * Nt, D] with c_remap = (g, Nt, 1), bias, aux = pos [g, D] read at row m % g: token rows = product + bias + pos,
    class-token rows and the allocation around the buffer bit-unchanged; on the 128 kernel, the 256 kernel and with split-K forced"""
    from unmore_amd import ops
    dev = _dev()
    B, g, D, K, tile, force = case
    args, kw, big = C.build_patch_embed(case, dtype, dev)
    umr_opts.setenv("UMR_GEMM_TILE", str(tile))
    if force:
        _force_split_k(ops, umr_opts, monkeypatch, force)
    if tile == 256:
        assert ops.gemm_nt(args[0], args[1], None, query_rowreduce=True), "the shape must run on the 256x256 kernels"
    rows = C._map_rows(torch.arange(B * g, device=dev), kw["c_remap"])
    _c_side(ops, args, kw, big, dtype, K, rows, force)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", C.PATCH_CASES[:2], ids=lambda c: "x".join(map(str, c[:4])))
def test_nt_hook_grad_token_rows(case, dtype, f32_mode_restored):
    """hook_grad's first call: out = dx, aux = dx (the same buffer), c_remap = (g, Nt, 1): token rows = old + product, class rows unchanged"""
    from unmore_amd import ops
    dev = _dev()
    B, g, D, K = case[:4]
    args, kw, big = C.build_hook_grad_tokens(case, dtype, dev)
    assert kw["out"].data_ptr() == kw["aux"].data_ptr()
    rows = C._map_rows(torch.arange(B * g, device=dev), kw["c_remap"])
    _c_side(ops, args, kw, big, dtype, K, rows)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,D,force", [(3, 128, None), (130, 128, "2"), (3, 200, None), (130, 200, None)])
def test_nt_hook_grad_class_rows(B, D, force, dtype, umr_opts, f32_mode_restored, monkeypatch):
    """hook_grad's second call: out = aux = cls_rows = dx.view(B, Nt * D)[:, :D] (ldc = ldaux = Nt * D): row 0 of every image = old +
    product, every other row of dx bit-unchanged; one case with split-K forced"""
    from unmore_amd import ops
    dev = _dev()
    args, kw, big = C.build_hook_grad_cls(B, D, dtype, dev)
    if force:
        _force_split_k(ops, umr_opts, monkeypatch, force)
    assert kw["out"].stride(0) == 37 * D
    _c_side(ops, args, kw, big, dtype, D, None, force)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [3, 130])
def test_nt_readout_class_token_half(B, dtype, f32_mode_restored):
    """gemm_nt(tok, w_full[:, D:], bias, M=B, lda=Nt*D, out_f32=True): A = the class-token row of every image (the token rows
    between them are NaN), B = a column slice of the [D, 2D] weight (its other half is NaN), f32 output"""
    from unmore_amd import ops
    dev = _dev()
    args, kw = C.build_readout_cls(B, dtype, dev)
    ref, _ = C.ref_gemm_nt(*args, **kw)
    big, out = C.sentinel(B, 128, F32, dev)
    before = big.clone()
    for mode in _modes(dtype, 128):
        _set_mode(mode)
        big.copy_(before)
        ops.gemm_nt(*args, **kw, out=out)
        _assert_rest_untouched(big, before, out)
        _close(out, ref, dtype)


# ------------------------------------------------------------------------------------------------ narrow / odd outputs
def _narrow(ops, combo, dtype, dev, idx):
    N, M, K = combo[:3]
    args, kw, bigs = C.build_narrow(combo, dtype, dev, idx)
    before = [b.clone() if b is not None else None for b in bigs]
    ref, ref2 = C.ref_gemm_nt(*args, **kw)
    for mode in _modes(dtype, K):
        _set_mode(mode)
        for b, b0 in zip(bigs, before):
            if b is not None:
                b.copy_(b0)
        ops.gemm_nt(*args, **kw)
        _close(kw["out"], ref, dtype)
        _assert_rest_untouched(bigs[0], before[0], kw["out"])
        if kw["c2_mode"]:
            _close(kw["out2"], ref2, dtype)
            _assert_rest_untouched(bigs[1], before[1], kw["out2"])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("idx", range(len(C.NARROW_COMBOS)), ids=lambda i: "-".join(map(str, C.NARROW_COMBOS[i])))
def test_nt_narrow_outputs_activations_aux2(idx, dtype, f32_mode_restored):
    """The scalar branches of epilogue_store (N = 1, 2, 6: no full vector; 12, 100: N % 8 != 0) and, with N = 96 / 200, the vector
    epilogues, through a fixed list of activation x bias x aux kind x aux2 x c2_mode x out_f32; every [M, N] operand is a column
    slice of a wider allocation"""
    from unmore_amd import ops
    _narrow(ops, C.NARROW_COMBOS[idx], dtype, _dev(), idx)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N", [(1, 1), (5, 1), (130, 2)])
def test_nt_classifier_head_form(B, N, dtype, f32_mode_restored):
    """the classifier's output layer (binary_classifier.py: logits [B, 1] -> sigmoid, f32 output): K = 8, one or two columns"""
    from unmore_amd import ops
    args, kw, big = C.build_classifier_head(B, N, dtype, _dev())
    before = big.clone()
    ref, _ = C.ref_gemm_nt(*args, **kw)
    for mode in _modes(dtype, 8):
        _set_mode(mode)
        big.copy_(before)
        ops.gemm_nt(*args, **kw)
        _assert_rest_untouched(big, before, kw["out"])
        _close(kw["out"], ref, dtype)


# ------------------------------------------------------------------------------------------------ TN gathers
def _tn_out(kw):
    return [kw["dW"]] + ([kw["dbias"]] if kw.get("dbias") is not None else [])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("way", C.TN_WAYS)
@pytest.mark.parametrize("case", C.TN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tn_row_gathers(case, way, dtype, umr_opts, f32_mode_restored):
    """Weight gradients over gathered rows (x_remap: the readout weight; dy_remap + dbias: the patch embedding; both; accumulate):
    split boundaries inside an image, the M > 4096 plan, tiny N and K.  Against float64 -- dbias over the addressed rows only --,
    bit for bit against the compact-operand call, and again with the 256 tile requested (a remapped call must fall back)."""
    from unmore_amd import ops
    dev = _dev()
    kw, ck, big = C.build_tn(case, way, dtype, dev)
    before = big.clone()
    prior = [t.clone() for t in _tn_out(kw)]
    refw, refb = C.ref_gemm_tn(**kw)
    for mode in (("x3", "exact") if dtype == F32 else (None,)):
        _set_mode(mode)
        res = {}
        for tile in ("128", "256"):
            umr_opts.setenv("UMR_GEMM_TILE", tile)
            for t, p in zip(_tn_out(kw), prior):
                t.copy_(p)
            ops.gemm_tn(**kw)
            res[tile] = [t.clone() for t in _tn_out(kw)]
            _assert_rest_untouched(big, before, kw["dW"])
        umr_opts.setenv("UMR_GEMM_TILE", "128")
        for t, p in zip(_tn_out(ck), prior):
            t.copy_(p)
        ops.gemm_tn(**ck)
        _close(res["128"][0], refw, dtype)
        if refb is not None:
            _close(res["128"][1], refb, dtype)
        for a, b, c in zip(res["128"], res["256"], _tn_out(ck)):
            assert _same_bits(a, c), (mode, "remapped and compact operands differ")
            assert _same_bits(a, b), (mode, "a remapped call changed with UMR_GEMM_TILE=256")


def test_tn_planes_refuse_row_remaps():
    """dtype UMR_BF16X3 has no row remaps (include/umr.h): the call raises and writes nothing"""
    from unmore_amd import ops
    dev = _dev()
    B, g, Nt, N, K = 3, 20, 21, 8, 16
    dY = C.rnd((B * Nt, 3 * N), BF16, dev, 1)
    X = C.rnd((B * g, 3 * K), BF16, dev, 2)
    big, dW = C.sentinel(N, K, F32, dev, 4, 4)
    before = big.clone()
    with pytest.raises(RuntimeError):
        ops.gemm_tn(dY, X, dW=dW, dy_remap=(g, Nt, 1), M=B * g, x3=True)
    with pytest.raises(RuntimeError):
        ops.gemm_tn(C.rnd((B * g, 3 * N), BF16, dev, 3), C.rnd((B * Nt, 3 * K), BF16, dev, 4), dW=dW, x_remap=(g, Nt, 1), M=B * g, x3=True)
    torch.cuda.synchronize()
    _assert_rest_untouched(big, before)


# ------------------------------------------------------------------------------------------------ one small call per engine form
def _planes_to_f64(pl, N):
    return pl[..., :N].double() + pl[..., N:2 * N].double() + pl[..., 2 * N:].double()


_NT_FORMS = sorted(f for f, t in C.COVERED.items() if t == C._G + "test_nt_engine_form")
_TN_FORMS = sorted(f for f, t in C.COVERED.items() if t == C._G + "test_tn_engine_form")


@pytest.mark.parametrize("form", _NT_FORMS, ids=lambda f: "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in f))
def test_nt_engine_form(form, f32_mode_restored):
    """A form the engine launches that no other kernel test has as a whole: a small problem of exactly that signature (two row tiles,
    image ends inside a tile, N = 72) against float64; rows a C remap skips stay as they were"""
    from unmore_amd import ops
    dev = _dev()
    args, kw, rargs, rkw = C.build_nt_of_form(form, dev)
    planes = form.kind == "planes"
    if planes:
        args = (ops.split3(args[0]), ops.split3(args[1]), args[2])
    assert C.form_of_nt(*args, planes=planes, **kw) == form
    dtype = BF16 if form.kind == "bf16" else F32
    ref, ref2 = C.ref_gemm_nt(*rargs, **rkw)
    out0 = kw["out"].clone() if "out" in kw else None
    for mode in ((None,) if dtype == BF16 else ("x3", "exact")):
        _set_mode(mode)
        if out0 is not None:
            kw["out"].copy_(out0)
        if planes:
            got = _tuple(ops.gemm_nt_x3(*args, **kw))
            got = tuple(_planes_to_f64(t, args[1].shape[0]) if t.dtype == BF16 else t for t in got)
        else:
            got = _tuple(ops.gemm_nt(*args, **kw))
        _close(got[0], ref, dtype)
        if form.c2:
            _close(got[1], ref2, dtype)


@pytest.mark.parametrize("form", _TN_FORMS, ids=lambda f: "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in f))
def test_tn_engine_form(form, f32_mode_restored):
    """the same for the weight-gradient descriptor"""
    from unmore_amd import ops
    dev = _dev()
    kw = C.build_tn_of_form(form, dev)
    planes = form.kind == "planes"
    dtype = BF16 if form.kind == "bf16" else F32
    refw, refb = C.ref_gemm_tn(**kw)
    prior = [t.clone() for t in _tn_out(kw)]
    for mode in ((None,) if dtype == BF16 else ("x3", "exact")):
        _set_mode(mode)
        for t, p in zip(_tn_out(kw), prior):
            t.copy_(p)
        if planes:
            pk = dict(kw, dY=ops.split3(kw["dY"]), X=ops.split3(kw["X"]), x3=True)
            assert C.form_of_tn(**pk) == form
            ops.gemm_tn(**pk)
        else:
            assert C.form_of_tn(**kw) == form
            ops.gemm_tn(**kw)
        _close(kw["dW"], refw, dtype)
        if refb is not None:
            _close(kw["dbias"], refb, dtype)


# ------------------------------------------------------------------------------------------------ inventory
def _record(monkeypatch, seen):
    from unmore_amd import ops
    nt, ntx, tn = ops.gemm_nt, ops.gemm_nt_x3, ops.gemm_tn

    def rec_nt(*a, **k):
        seen.add(C.form_of_nt(*a, **k))
        return nt(*a, **k)

    def rec_ntx(*a, **k):
        seen.add(C.form_of_nt(*a, planes=True, **k))
        return ntx(*a, **k)

    def rec_tn(*a, **k):
        seen.add(C.form_of_tn(*a, **k))
        return tn(*a, **k)

    monkeypatch.setattr(ops, "gemm_nt", rec_nt)
    monkeypatch.setattr(ops, "gemm_nt_x3", rec_ntx)
    monkeypatch.setattr(ops, "gemm_tn", rec_tn)


def engine_forms(monkeypatch):
    """the signatures of every GEMM call of one TrainStep.step on dpt_tiny (B = 2, 64 x 96; f32 and bf16) and of one prediction of
    the existence classifier (f32 and bf16)"""
    from argparse import Namespace
    from oracle import classifier_oracle as CO
    from unmore_amd import synth
    from unmore_amd.binary_classifier import Binary_Classifier
    from unmore_amd.hashrng import hash_init, uniform, uniform01
    from unmore_amd.objectness_net import ObjectnessNet
    from unmore_amd.trainer import TrainStep
    seen = set()
    _record(monkeypatch, seen)
    batch = [torch.from_numpy(a).cuda() for a in synth.make_batch(2, 64, 96, seed=3)]
    for dtype in (F32, BF16):
        net = ObjectnessNet("cuda:0", 64, "dpt_tiny", Namespace(use_bg_sdf=True, sdf_activation="tanh"))
        net.load_state_dict({k: torch.from_numpy(hash_init(k, tuple(v.shape), "tiny")) for k, v in net.state_dict().items()}, strict=True)
        net = net.to("cuda:0")
        net.set_compute_dtype(dtype)
        out5 = TrainStep(net, lr=1e-4).step(*batch)
        assert bool(torch.isfinite(out5).all())
        clf = Binary_Classifier(device="cuda:0", image_size=128, args=None, compute_dtype=dtype)
        clf.load_state_dict(CO.hash_state("clf", uniform), strict=True)
        clf = clf.to("cuda:0").eval()
        with torch.no_grad():
            y = clf(torch.from_numpy(uniform01("img:clf64", (2, 3, 64, 64))).cuda())
        assert y.shape == (2, 1) and bool(torch.isfinite(y).all())
    torch.cuda.synchronize()
    return seen


def test_every_engine_form_is_pinned(monkeypatch):
    """Keeps the suite honest: a change that makes the engine launch a GEMM form no kernel test pins fails here until
    gemm_forms_common.COVERED names the test that does"""
    seen = engine_forms(monkeypatch)
    assert len(seen) > 10
    missing = sorted(map(repr, seen - set(C.COVERED)))
    assert not missing, "GEMM forms the engine launches that no kernel test pins (gemm_forms_common.COVERED):\n" + "\n".join(missing)
