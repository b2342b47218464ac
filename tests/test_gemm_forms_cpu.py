"""The float64 restatement of the GEMM descriptors (gemm_forms_common.py) is right -- against loops written out by hand --, the
inputs of test_gemm_forms_gpu.py tell a wrong row map, a dropped operand or a swapped epilogue step from the right one by more than
the tolerance the GPU test applies, and every entry of COVERED names a test that exists.  No GPU."""
import ast
import math
import os

import pytest
import torch

import gemm_forms_common as C

F32, BF16 = torch.float32, torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))


def test_activation_codes_are_the_librarys():
    from unmore_amd import _lib as L
    assert (C.ACT_NONE, C.ACT_RELU, C.ACT_GELU, C.ACT_TANH, C.ACT_SIGMOID) == (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU, L.ACT_TANH, L.ACT_SIGMOID)


# ------------------------------------------------------------------------------------------------ against hand-written loops
def _gelu(x):
    return 0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0)))


def _dgelu(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0))) + x * math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


_ACTS = {C.ACT_NONE: lambda x: x, C.ACT_RELU: lambda x: max(x, 0.0), C.ACT_GELU: _gelu, C.ACT_TANH: math.tanh,
         C.ACT_SIGMOID: lambda x: 1.0 / (1.0 + math.exp(-x))}


@pytest.mark.parametrize("akind", ["add", "mask", "dgelu"])
@pytest.mark.parametrize("act,c2", [(C.ACT_GELU, 2), (C.ACT_TANH, 1), (C.ACT_SIGMOID, 0), (C.ACT_RELU, 2)])
def test_ref_gemm_nt_against_loops(akind, act, c2):
    """every part of the descriptor at once: A gathered past a skipped row per image with lda > K, C / C2 / aux2 scattered past two
    skipped rows per image with ldc > N, aux broadcast over images, row bias per image"""
    Bn, g, N, K = 3, 4, 3, 2
    a_nt, c_nt, lda, ldc = 5, 6, 3, 5
    A = C.rnd((Bn * a_nt, lda), F32, "cpu", 1)
    W = C.rnd((N, K), F32, "cpu", 2)
    bias = C.rnd((N,), F32, "cpu", 3)
    rb = C.rnd((Bn, N), F32, "cpu", 4)
    aux = C.rnd((g, N), F32, "cpu", 5)
    aux2 = C.rnd((Bn * c_nt, N), F32, "cpu", 6)
    outb = C.rnd((Bn * c_nt, ldc), F32, "cpu", 7)
    out2b = C.rnd((Bn * c_nt, ldc), F32, "cpu", 8)
    out, out2 = outb[:, 1:1 + N], out2b[:, 2:2 + N]
    got, got2 = C.ref_gemm_nt(A[:, :K], W, bias, out=out, out2=out2 if c2 else None, aux=aux, aux2=aux2, rowbias=rb, rows_per_batch=g, act=act,
                              mask_relu=akind == "mask", mask_dgelu=akind == "dgelu", c2_mode=c2, M=Bn * g, a_remap=(g, a_nt, 1),
                              c_remap=(g, c_nt, 2), aux_mod=g)
    want, want2 = out.double().clone(), out2.double().clone()
    for m in range(Bn * g):
        ar = (m // g) * a_nt + 1 + m % g
        cr = (m // g) * c_nt + 2 + m % g
        for n in range(N):
            v = sum(float(A[ar, k]) * float(W[n, k]) for k in range(K)) + float(bias[n]) + float(rb[m // g, n])
            a = float(aux[m % g, n])
            v = v + a if akind == "add" else (v if a > 0 else 0.0) if akind == "mask" else v * _dgelu(a)
            v += float(aux2[cr, n])
            if c2 == 2:
                want2[cr, n] = v
            v = _ACTS[act](v)
            want[cr, n] = v
            if c2 == 1:
                want2[cr, n] = max(v, 0.0)
    torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12)
    if c2:
        torch.testing.assert_close(got2, want2, atol=1e-12, rtol=1e-12)
    else:
        assert got2 is None
    # the class-token form: M rows at a stride of several rows (lda = a_nt * lda elements), no remap
    got, _ = C.ref_gemm_nt(A[:, :K], W, None, M=Bn, lda=a_nt * lda)
    for b in range(Bn):
        for n in range(N):
            assert abs(float(got[b, n]) - sum(float(A[b * a_nt, k]) * float(W[n, k]) for k in range(K))) < 1e-12


@pytest.mark.parametrize("accumulate", [False, True])
def test_ref_gemm_tn_against_loops(accumulate):
    Bn, g, N, K = 3, 4, 3, 2
    y_nt, x_nt, lddy, ldx = 5, 6, 4, 5
    dY = C.rnd((Bn * y_nt, lddy), F32, "cpu", 11)
    X = C.rnd((Bn * x_nt, ldx), F32, "cpu", 12)
    dW0, db0 = C.rnd((N, K), F32, "cpu", 13), C.rnd((N,), F32, "cpu", 14)
    w, b = C.ref_gemm_tn(dY[:, 1:1 + N], X[:, 2:2 + K], dW=dW0, dbias=db0, accumulate=accumulate, M=Bn * g, dy_remap=(g, y_nt, 1),
                         x_remap=(g, x_nt, 2))
    for n in range(N):
        sb = float(db0[n]) if accumulate else 0.0
        for k in range(K):
            s = float(dW0[n, k]) if accumulate else 0.0
            for m in range(Bn * g):
                s += float(dY[(m // g) * y_nt + 1 + m % g, 1 + n]) * float(X[(m // g) * x_nt + 2 + m % g, 2 + k])
            assert abs(float(w[n, k]) - s) < 1e-12
        for m in range(Bn * g):
            sb += float(dY[(m // g) * y_nt + 1 + m % g, 1 + n])
        assert abs(float(b[n]) - sb) < 1e-12
    w2, b2 = C.ref_gemm_tn(dY[:, 1:1 + N], X[:, 2:2 + K], M=Bn * g, dy_remap=(g, y_nt, 1), x_remap=(g, x_nt, 2))
    assert b2 is None and w2.shape == (N, K)


def test_ref_conv_forms_are_torchs():
    """conv != 0: A is NHWC, B is [N][3][3][Cin]; the weight gradient is the adjoint of the forward"""
    x = C.rnd((2, 5, 4, 3), F32, "cpu", 21)
    w = C.rnd((6, 27), F32, "cpu", 22)
    for conv in (1, 2):
        y, _ = C.ref_gemm_nt(x, w, None, conv=conv)
        dy = C.rnd(tuple(y.shape), F32, "cpu", 23)
        dw, _ = C.ref_gemm_tn(dy, x, conv=conv)
        assert abs(float((y * dy.double()).sum()) - float((dw * w.double()).sum())) < 1e-9
    # the centre tap of an interior pixel, by hand
    y, _ = C.ref_gemm_nt(x, w, None, conv=1)
    want = sum(float(x[0, 1 + ky, 1 + kx, c]) * float(w[2, (ky * 3 + kx) * 3 + c]) for ky in range(3) for kx in range(3) for c in range(3))
    assert abs(float(y.view(2, 5, 4, 6)[0, 2, 2, 2]) - want) < 1e-12


# ------------------------------------------------------------------------------------------------ the inputs discriminate
def _moved(a, b, dtype):
    return any(x is not None and not C.within(x, y, dtype) for x, y in zip(a, b))


def _nt_faults(args, kw, dtype, faults):
    good = C.ref_gemm_nt(*args, **kw)
    assert all(bool(torch.isfinite(t).all()) for t in good if t is not None), "the right rows hold no NaN"
    for f in faults:
        assert f in C.FAULTS_NT
        assert _moved(C.ref_gemm_nt(*args, fault=f, **kw), good, dtype), f"fault '{f}' stays within the tolerance of the GPU test"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", C.GATHER_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gather_inputs_show_row_faults(case, dtype):
    args, kw, compact = C.build_gather(case, dtype, "cpu", False)
    _nt_faults(args, kw, dtype, ("row_off_plus_one", "rows_out_is_rows_in"))
    ckw = {k: v for k, v in kw.items() if k not in ("M", "a_remap")}
    assert torch.equal(C.ref_gemm_nt(compact, args[1], None, **ckw)[0], C.ref_gemm_nt(*args, **kw)[0])
    args, kw, _ = C.build_gather(case, dtype, "cpu", True)
    _nt_faults(args, kw, dtype, ("row_off_plus_one", "rows_out_is_rows_in", "rowbias_by_remapped_row", "act_before_c2"))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", C.PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_c_side_inputs_show_row_faults(case, dtype):
    args, kw, _ = C.build_patch_embed(case, dtype, "cpu")
    _nt_faults(args, kw, dtype, ("row_off_plus_one", "rows_out_is_rows_in", "aux_row_is_m"))
    args, kw, _ = C.build_hook_grad_tokens(case, dtype, "cpu")
    _nt_faults(args, kw, dtype, ("row_off_plus_one", "rows_out_is_rows_in"))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_narrow_inputs_show_epilogue_faults(dtype):
    n_aux2 = n_c2 = 0
    for idx, combo in enumerate(C.NARROW_COMBOS):
        args, kw, _ = C.build_narrow(combo, dtype, "cpu", idx)
        faults = []
        if combo[6]:
            faults.append("aux2_dropped")
            n_aux2 += 1
        if combo[7] == 2 and combo[3] != C.ACT_NONE:
            faults.append("act_before_c2")
            n_c2 += 1
        _nt_faults(args, kw, dtype, faults)
    assert n_aux2 >= 10 and n_c2 >= 10


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("way", C.TN_WAYS)
@pytest.mark.parametrize("case", C.TN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tn_inputs_show_row_faults(case, way, dtype):
    kw, ck, _ = C.build_tn(case, way, dtype, "cpu")
    good = C.ref_gemm_tn(**kw)
    assert all(bool(torch.isfinite(t).all()) for t in good if t is not None)
    same = C.ref_gemm_tn(**ck)
    torch.testing.assert_close(same[0], good[0], atol=1e-12, rtol=1e-12)   # the compact call is the same problem
    for f in ("row_off_plus_one", "rows_out_is_rows_in") + (("dbias_all_rows",) if way != 1 else ()):
        assert f in C.FAULTS_TN
        assert _moved(C.ref_gemm_tn(fault=f, **kw), good, dtype), f"fault '{f}' stays within the tolerance of the GPU test"


def test_narrow_combos_cover_the_sets_they_are_drawn_from():
    assert len(C.NARROW_COMBOS) == 56 and len(set(C.NARROW_COMBOS)) == 56
    for i, (N, M, K, act, bias, akind, aux2, c2, out_f32) in enumerate(C.NARROW_COMBOS):
        assert N in ((1, 2, 6, 12, 100) if i < 48 else (96, 200)) and M in (1, 130) and K in (8, 136)
        assert act in _ACTS and akind in ("none", "add", "mask", "dgelu") and c2 in (0, 1, 2)
    for col, values in ((0, (1, 2, 6, 12, 100)), (3, tuple(_ACTS)), (5, ("none", "add", "mask", "dgelu")), (7, (0, 1, 2))):
        assert {c[col] for c in C.NARROW_COMBOS[:48]} == set(values)


# ------------------------------------------------------------------------------------------------ the table of pinned forms
def _test_functions(fname):
    with open(os.path.join(HERE, fname)) as f:
        tree = ast.parse(f.read())
    return {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_covered_names_tests_that_exist():
    assert C.COVERED
    files = {}
    for form, where in C.COVERED.items():
        assert isinstance(form, (C.NTForm, C.TNForm)), form
        fname, _, func = where.partition("::")
        assert fname.startswith("test_") and fname.endswith("_gpu.py"), where
        if fname not in files:
            files[fname] = _test_functions(fname)
        assert func in files[fname], f"{where}: no such test"


def test_the_new_tests_run_the_forms_they_are_cited_for():
    """the inputs of a dedicated test of test_gemm_forms_gpu.py have the signature COVERED cites that test for"""
    hit = set()

    def cited(form, name):
        assert form in C.COVERED, (name, form)
        assert C.COVERED[form] == C._G + name, (name, form)
        hit.add(C._G + name)

    for dtype in (F32, BF16):
        args, kw, _ = C.build_gather(C.GATHER_CASES[0], dtype, "cpu", True)
        if dtype == BF16:   # the fp32 engine compacts the token rows into planes instead
            cited(C.form_of_nt(*args, **kw), "test_nt_a_row_gather")
        args, kw, _ = C.build_patch_embed(C.PATCH_CASES[0], dtype, "cpu")
        if dtype == BF16:
            cited(C.form_of_nt(*args, **kw), "test_nt_patch_embed_form")
        args, kw, _ = C.build_hook_grad_tokens(C.PATCH_CASES[0], dtype, "cpu")
        if dtype == BF16:
            cited(C.form_of_nt(*args, **kw), "test_nt_hook_grad_token_rows")
        args, kw, _ = C.build_hook_grad_cls(3, 128, dtype, "cpu")
        cited(C.form_of_nt(*args, **kw), "test_nt_hook_grad_class_rows")
        args, kw = C.build_readout_cls(3, dtype, "cpu")
        cited(C.form_of_nt(*args, **kw), "test_nt_readout_class_token_half")
        args, kw, _ = C.build_classifier_head(5, 1, dtype, "cpu")
        cited(C.form_of_nt(*args, **kw), "test_nt_classifier_head_form")
        kw, _, _ = C.build_tn(C.TN_CASES[0], 1, dtype, "cpu")
        if dtype == BF16:
            cited(C.form_of_tn(**kw), "test_tn_row_gathers")
    own = {t for t in C.COVERED.values() if t.startswith(C._G)} - {C._G + "test_nt_engine_form", C._G + "test_tn_engine_form"}
    assert hit == own, own - hit


def test_small_calls_have_the_form_they_are_built_for():
    """test_nt_engine_form / test_tn_engine_form run build_*_of_form(form): the call it returns has that signature"""
    for form, where in C.COVERED.items():
        if where == C._G + "test_nt_engine_form":
            args, kw, rargs, rkw = C.build_nt_of_form(form, "cpu")
            planes = form.kind == "planes"
            if planes:   # the plane operands' shapes, without the library's split
                args = tuple(torch.cat([t, t, t], -1).to(BF16) if i < 2 else t for i, t in enumerate(args))
            assert C.form_of_nt(*args, planes=planes, **kw) == form
            ref, ref2 = C.ref_gemm_nt(*rargs, **rkw)
            assert bool(torch.isfinite(ref).all()) and (ref2 is None) == (form.c2 == 0)
        elif where == C._G + "test_tn_engine_form":
            kw = C.build_tn_of_form(form, "cpu")
            pk = dict(kw, dY=torch.cat([kw["dY"]] * 3, -1).to(BF16), X=torch.cat([kw["X"]] * 3, -1).to(BF16), x3=True) if form.kind == "planes" else kw
            assert C.form_of_tn(**pk) == form
            w, b = C.ref_gemm_tn(**kw)
            assert bool(torch.isfinite(w).all()) and (b is None) == (not form.dbias)
