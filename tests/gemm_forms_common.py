"""Float64 restatement of umr_gemm_desc / umr_gemm_tn_desc (include/umr.h) for the tests (no test file of its own: imported by
test_gemm_forms_*.py), the signature ("form") of a GEMM call, the table of forms a kernel test pins, and the seeded inputs the GPU
tests run -- built here so that the CPU tests can show, on the very same inputs, that a wrong row map would be seen.

Plain torch, device-agnostic: the GPU tests hand the device tensors themselves to the restatement (strides, aliasing and the
allocation around a view are part of what a descriptor says), the CPU tests build the same inputs with dev="cpu"."""
import collections
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 5   # enum umr_act
NAN = float("nan")
PAD = 256   # rows of NaN (inputs) / sentinel (outputs) before and after every remapped or strided operand

FAULTS_NT = ("row_off_plus_one", "rows_out_is_rows_in", "aux_row_is_m", "rowbias_by_remapped_row", "aux2_dropped", "act_before_c2")
FAULTS_TN = ("row_off_plus_one", "rows_out_is_rows_in", "dbias_all_rows")


def tol(dtype):
    """the project's GEMM tolerance against float64 (tests/test_gemm_gpu.py::_tol)"""
    return dict(atol=2e-5, rtol=2e-5) if dtype == torch.float32 else dict(atol=3e-2, rtol=3e-2)


def within(x, ref, dtype):
    """x within tol(dtype) of ref everywhere (a NaN on either side is outside)"""
    t = tol(dtype)
    return bool(torch.allclose(x.double(), ref.double(), atol=t["atol"], rtol=t["rtol"]))


# ------------------------------------------------------------------------------------------------ the restatement
def _map_rows(m, remap, fault=None):
    """logical rows m -> (m // rows_in) * rows_out + row_off + m % rows_in (0 / None = identity)"""
    if remap is None or remap[0] <= 0:
        return m
    ri, ro, off = remap
    if fault == "row_off_plus_one":
        off += 1
    if fault == "rows_out_is_rows_in":
        ro = ri
    return (m // ri) * ro + off + m % ri


def _rows_at(t, ld, idx, ncols):
    """rows idx ([n] int64) of the row-major operand that starts at t's first element with row stride ld"""
    flat = t.as_strided((int(idx.max()) + 1, ncols), (ld, 1), t.storage_offset())
    return flat[idx.to(t.device)]


def _view2d(t, ncols):
    return t if t.dim() == 2 else t.reshape(-1, ncols)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act64(v, act):
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_GELU:
        return gelu64(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    assert act == ACT_NONE, act
    return v


def ref_gemm_nt(A, B, bias=None, *, out=None, out2=None, aux=None, aux2=None, rowbias=None, rows_per_batch=0, act=ACT_NONE,
                mask_relu=False, mask_dgelu=False, c2_mode=0, out_f32=False, conv=0, M=None, lda=None, a_remap=None, c_remap=None,
                aux_mod=0, fault=None):
    """ops.gemm_nt in float64, same keywords.  Returns (C, C2): the FULL buffers `out` / `out2` (as 2-D [rows, N] float64, the rows a
    C remap leaves alone included; zeros where no buffer was given), C2 None without c2_mode.  Operands are read as the tensors hold
    them (already rounded to the compute dtype).  Order (include/umr.h): + bias, + rowbias[m_logical // rows_per_batch], aux (add /
    keep where > 0 / times GELU'), + aux2, C2 (mode 2) = v, act, C = v, C2 (mode 1) = relu(v).
    fault: one of FAULTS_NT -- a deliberately wrong restatement, for the tests that show the inputs discriminate."""
    dev = A.device
    N, K = B.shape
    Bd = B.double()
    if conv:
        nb, H, W, Cin = A.shape
        s = 2 if conv == 2 else 1
        w = Bd.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2)
        acc = F.conv2d(A.double().permute(0, 3, 1, 2), w, None, stride=s, padding=1).permute(0, 2, 3, 1).reshape(-1, N)
        Mv = acc.shape[0]
        m = torch.arange(Mv, device=dev)
    else:
        A2 = _view2d(A, A.shape[-1])
        Mv = A2.shape[0] if M is None else M
        m = torch.arange(Mv, device=dev)
        ar = _map_rows(m, a_remap, fault)
        acc = _rows_at(A2, A2.stride(0) if lda is None else lda, ar, K).double() @ Bd.t()
    cm = _map_rows(m, c_remap, fault)
    if fault is not None and out is not None:   # a wrong map may leave the buffer: keep the wrong restatement inside it
        cm = cm.clamp(max=_view2d(out, N).shape[0] - 1)
    v = acc
    if bias is not None:
        v = v + bias.double()
    if rowbias is not None:
        rrow = m
        if fault == "rowbias_by_remapped_row":
            rrow = _map_rows(m, c_remap if c_remap is not None else a_remap)
        v = v + rowbias.double()[(rrow // rows_per_batch).clamp(max=rowbias.shape[0] - 1)]
    if aux is not None:
        aux2d = _view2d(aux, N)
        arow = (m % aux_mod) if aux_mod > 0 else cm
        if fault == "aux_row_is_m" and aux_mod > 0:
            arow = m.clamp(max=aux2d.shape[0] - 1)
        a = aux2d[arow].double()
        v = torch.where(a > 0, v, torch.zeros_like(v)) if mask_relu else (v * dgelu64(a) if mask_dgelu else v + a)
    if aux2 is not None and fault != "aux2_dropped":
        v = v + _view2d(aux2, N)[cm].double()
    rows_c = int(cm.max()) + 1
    C = _view2d(out, N).double().clone() if out is not None else torch.zeros((rows_c, N), dtype=torch.float64, device=dev)
    C2 = None
    if c2_mode:
        C2 = _view2d(out2, N).double().clone() if out2 is not None else torch.zeros((rows_c, N), dtype=torch.float64, device=dev)
    if c2_mode == 2:
        C2[cm] = act64(v, act) if fault == "act_before_c2" else v
    v = act64(v, act)
    C[cm] = v
    if c2_mode == 1:
        C2[cm] = F.relu(v)
    return C, C2


def ref_gemm_tn(dY, X, *, dW=None, dbias=None, accumulate=False, conv=0, M=None, dy_remap=None, x_remap=None, lddy=None, ldx=None,
                fault=None):
    """ops.gemm_tn in float64, same keywords (no x3: the plane operands' VALUES go through here as f32 tensors).  Returns (dW, dbias):
    dW[N, K] = sum over the M logical rows of dY[row]^T X[row], dbias = the column sums over the ADDRESSED dY rows only (None without
    a dbias buffer); with accumulate both are added to what the given buffers hold."""
    dev = X.device
    dY2 = _view2d(dY, dY.shape[-1])
    N = dY2.shape[1]
    Mv = dY2.shape[0] if M is None else M
    m = torch.arange(Mv, device=dev)
    yr = _rows_at(dY2, dY2.stride(0) if lddy is None else lddy, _map_rows(m, dy_remap, fault), N).double()
    if conv:
        nb, H, W, Cin = X.shape
        s = 2 if conv == 2 else 1
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        g = torch.nn.grad.conv2d_weight(X.double().permute(0, 3, 1, 2), (N, Cin, 3, 3), yr.view(nb, Ho, Wo, N).permute(0, 3, 1, 2),
                                        stride=s, padding=1)
        w = g.permute(0, 2, 3, 1).reshape(N, 9 * Cin)
    else:
        X2 = _view2d(X, X.shape[-1])
        K = X2.shape[1]
        xr = _rows_at(X2, X2.stride(0) if ldx is None else ldx, _map_rows(m, x_remap, fault), K).double()
        w = yr.t() @ xr
    b = None
    if dbias is not None:
        b = yr.sum(0)
        if fault == "dbias_all_rows":
            b = dY2.double().sum(0)
        if accumulate:
            b = b + dbias.double()
    if accumulate:
        w = w + dW.double()
    return w, b


# ------------------------------------------------------------------------------------------------ forms
NTForm = collections.namedtuple("NTForm", "kind conv act aux aux2 bias rowbias c2 out_f32 a_remap c_remap aux_mod lda ldc alias red no_store")
TNForm = collections.namedtuple("TNForm", "kind conv dbias accumulate dy_remap x_remap lddy ldx")


def _kind(t, planes):
    return "planes" if planes else {torch.float32: "f32", torch.bfloat16: "bf16"}[t.dtype]


def form_of_nt(A, B, bias=None, *, planes=False, out=None, out2=None, aux=None, aux2=None, rowbias=None, rows_per_batch=0, act=ACT_NONE,
               mask_relu=False, mask_dgelu=False, mask=None, dgelu=None, c2_mode=0, out_f32=False, out_planes=False, c2_planes=False,
               conv=0, M=None, lda=None, a_remap=None, c_remap=None, aux_mod=0, red_w=None, no_store=False, **_queries):
    """Signature of an ops.gemm_nt call, or (planes=True) of an ops.gemm_nt_x3 call: which optional parts of umr_gemm_desc it uses.
    Shapes and values do not enter; strides enter only as "larger than the row"."""
    pl = 3 if planes else 1
    N, K = B.shape[0], B.shape[1] // pl
    if planes:
        a_t, akind = (mask, "mask") if mask is not None else ((dgelu, "dgelu") if dgelu is not None else (aux, "add"))
        out_f32 = red_w is None and not (out_planes or (out is not None and out.dtype == torch.bfloat16))
    else:
        a_t, akind = aux, ("mask" if mask_relu else ("dgelu" if mask_dgelu else "add"))
    if a_t is None:
        akind = "none"
    strided_a = strided_c = False
    if not conv:
        A2 = _view2d(A, A.shape[-1])
        strided_a = (A2.stride(0) if lda is None else lda) != pl * K
    if out is not None:
        o2 = out if out.dim() == 2 else out.reshape(-1, out.shape[-1])
        strided_c = o2.stride(0) != o2.shape[1]
    alias = out is not None and a_t is not None and out.data_ptr() == a_t.data_ptr()
    return NTForm(_kind(A, planes), int(conv), int(act), akind, aux2 is not None, bias is not None, rowbias is not None, int(c2_mode),
                  bool(out_f32), a_remap is not None, c_remap is not None, aux_mod > 0, strided_a, strided_c, alias, red_w is not None,
                  bool(no_store) or (planes and red_w is not None))


def form_of_tn(dY, X, *, dW=None, dbias=None, accumulate=False, conv=0, M=None, dy_remap=None, x_remap=None, lddy=None, ldx=None, x3=False):
    """Signature of an ops.gemm_tn call"""
    pl = 3 if x3 else 1
    dY2 = _view2d(dY, dY.shape[-1]) if dY.is_contiguous() else dY
    strided_y = (dY2.stride(0) if lddy is None else lddy) != dY2.shape[-1]
    strided_x = False
    if not conv:
        X2 = _view2d(X, X.shape[-1]) if X.is_contiguous() else X
        strided_x = (X2.stride(0) if ldx is None else ldx) != X2.shape[-1]
    assert dY2.shape[-1] % pl == 0
    return TNForm(_kind(X, x3), int(conv), dbias is not None, bool(accumulate), dy_remap is not None, x_remap is not None, strided_y,
                  strided_x)


# ------------------------------------------------------------------------------------------------ inputs
def rnd(shape, dtype, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def poisoned(data, dev, col_lo=0, col_hi=0, fill=NAN):
    """`data` ([rows, cols], CPU) as a view into the middle of a larger allocation filled with NaN (an input) or with a sentinel (an
    output): PAD rows before and after, col_lo / col_hi columns left and right.  Returns (allocation, view), both on dev."""
    rows, cols = data.shape
    big = torch.full((PAD + rows + PAD, col_lo + cols + col_hi), fill, dtype=data.dtype)
    big[PAD:PAD + rows, col_lo:col_lo + cols] = data
    big = big.to(dev)
    return big, big[PAD:PAD + rows, col_lo:col_lo + cols]


def sentinel(rows, cols, dtype, dev, col_lo=0, col_hi=0):
    """an output buffer prefilled with a pattern no result comes near (-1000 - (r * 7 + c) % 32, rounded to dtype), inside a larger
    allocation of the same pattern: (allocation, view)"""
    R, Cc = PAD + rows + PAD, col_lo + cols + col_hi
    pat = -1000.0 - ((torch.arange(R).view(-1, 1) * 7 + torch.arange(Cc).view(1, -1)) % 32).float()
    big = pat.to(dtype).to(dev)
    return big, big[PAD:PAD + rows, col_lo:col_lo + cols]


def token_rows(B, g, Nt, off, cols, dtype, dev, seed, scale=1.0, col_lo=0, col_hi=0):
    """A token buffer [B*Nt, cols] whose rows off .. off+g-1 of every image hold data and every other row NaN, inside a NaN
    allocation: (allocation, view, the same g rows per image as a compact [B*g, cols] copy)."""
    data = torch.full((B, Nt, cols), NAN, dtype=dtype)
    compact = rnd((B * g, cols), dtype, "cpu", seed, scale)
    data[:, off:off + g] = compact.view(B, g, cols)
    big, view = poisoned(data.view(B * Nt, cols), dev, col_lo, col_hi)
    return big, view, compact.to(dev)


# ---- NT A-row gather (the readout form): (B, g, Nt, off, N, K), tile
GATHER_CASES = [(9, 36, 37, 1, 200, 136, 128), (60, 5, 6, 1, 64, 64, 128), (3, 200, 203, 2, 96, 128, 128), (2, 24, 25, 1, 128, 192, 128),
                (20, 36, 37, 1, 256, 128, 256), (3, 300, 301, 1, 192, 64, 256)]


def build_gather(case, dtype, dev, readout):
    """-> (args, kw, compact A): ops.gemm_nt(*args, **kw) gathers rows off .. off+g-1 of every image of a poisoned token buffer"""
    B, g, Nt, off, N, K, _ = case
    _, tok, compact = token_rows(B, g, Nt, off, K, dtype, dev, 101)
    W = rnd((N, K), dtype, dev, 102, K ** -0.5)
    kw = dict(M=B * g, a_remap=(g, Nt, off))
    if readout:
        kw.update(rowbias=rnd((B, N), torch.float32, dev, 103), rows_per_batch=g, act=ACT_GELU, c2_mode=2)
    return (tok, W, None), kw, compact


# ---- NT C side, patch-embed form: (B, g, D, K, tile, forced split-K)
PATCH_CASES = [(9, 36, 200, 136, 128, None), (60, 5, 64, 64, 128, None), (20, 36, 256, 128, 256, None), (9, 36, 200, 384, 128, "3")]


def build_patch_embed(case, dtype, dev):
    """-> (args, kw, allocation around `out`): rows written past a class-token row per image, position row m % g added"""
    B, g, D, K = case[:4]
    Nt = g + 1
    A = rnd((B * g, K), dtype, dev, 111)
    W = rnd((D, K), dtype, dev, 112, K ** -0.5)
    bias = rnd((D,), torch.float32, dev, 113)
    pos = rnd((g, D), dtype, dev, 114)
    big, tokens = sentinel(B * Nt, D, dtype, dev)
    return (A, W, bias), dict(out=tokens, aux=pos, aux_mod=g, c_remap=(g, Nt, 1)), big


def build_hook_grad_tokens(case, dtype, dev):
    """hook_grad's first call: dx[token rows] += d_rpre . W^T, out aliases aux, class-token rows untouched"""
    B, g, D, K = case[:4]
    Nt = g + 1
    A = rnd((B * g, K), dtype, dev, 121)
    W = rnd((D, K), dtype, dev, 122, K ** -0.5)
    big, dx = poisoned(rnd((B * Nt, D), dtype, "cpu", 123), dev, fill=-1000.0)
    return (A, W, None), dict(out=dx, aux=dx, c_remap=(g, Nt, 1)), big


def build_hook_grad_cls(B, D, dtype, dev, Nt=37):
    """hook_grad's second call: row 0 of every image of dx (row stride Nt * D) += sB . W^T, out aliases aux"""
    sB = rnd((B, D), dtype, dev, 131)
    W = rnd((D, D), dtype, dev, 132, D ** -0.5)
    big, dx = poisoned(rnd((B * Nt, D), dtype, "cpu", 133), dev, fill=-1000.0)
    cls_rows = dx.view(B, Nt * D)[:, :D]
    return (sB, W, None), dict(out=cls_rows, aux=cls_rows), big


def build_readout_cls(B, dtype, dev, Nt=37, D=128):
    """the readout's class-token half: A = row 0 of every image (lda = Nt * D; the token rows are NaN), B = the right half of the
    [D, 2D] weight (its left half is NaN), f32 output"""
    data = torch.full((B, Nt, D), NAN, dtype=dtype)
    data[:, 0] = rnd((B, D), dtype, "cpu", 141)
    _, tok = poisoned(data.view(B * Nt, D), dev)
    w_full = torch.full((D, 2 * D), NAN, dtype=dtype)
    w_full[:, D:] = rnd((D, D), dtype, "cpu", 142, D ** -0.5)
    w_full = w_full.to(dev)
    bias = rnd((D,), torch.float32, dev, 143)
    return (tok, w_full[:, D:], bias), dict(M=B, lda=Nt * D, out_f32=True)


# ---- narrow and odd outputs, activations, aux2: (N, M, K, act, bias, aux kind, aux2, c2_mode, out_f32).  Drawn once with
# random.Random(20240607) -- 48 distinct draws with N from {1, 2, 6, 12, 100}, then 8 with N from {96, 200} (the vector epilogues: the
# unrolled one and epilogue_store8) -- and fixed here, so that the list a failure names never moves
NARROW_COMBOS = [
    (100, 130, 136, ACT_NONE, False, "add", True, 1, True),
    (6, 1, 136, ACT_SIGMOID, True, "none", True, 2, True),
    (1, 1, 8, ACT_NONE, True, "mask", False, 2, True),
    (6, 130, 8, ACT_GELU, False, "mask", True, 1, True),
    (100, 130, 136, ACT_RELU, True, "mask", False, 2, False),
    (12, 1, 8, ACT_TANH, False, "dgelu", True, 1, False),
    (6, 130, 8, ACT_TANH, True, "none", True, 0, True),
    (12, 1, 136, ACT_RELU, True, "add", True, 2, False),
    (2, 1, 136, ACT_GELU, True, "add", True, 2, True),
    (12, 1, 8, ACT_SIGMOID, True, "none", True, 2, True),
    (12, 130, 8, ACT_GELU, True, "mask", False, 1, False),
    (6, 1, 136, ACT_NONE, False, "add", True, 0, False),
    (2, 130, 136, ACT_TANH, False, "add", False, 0, True),
    (2, 1, 136, ACT_RELU, False, "add", True, 0, True),
    (2, 1, 136, ACT_TANH, True, "mask", False, 0, True),
    (2, 1, 136, ACT_RELU, False, "dgelu", True, 0, False),
    (100, 1, 8, ACT_SIGMOID, True, "mask", True, 2, True),
    (12, 130, 136, ACT_GELU, False, "dgelu", False, 0, True),
    (6, 1, 136, ACT_GELU, False, "none", True, 1, True),
    (6, 1, 136, ACT_SIGMOID, True, "dgelu", True, 2, False),
    (100, 1, 8, ACT_RELU, False, "add", False, 2, False),
    (2, 1, 8, ACT_SIGMOID, False, "mask", True, 2, True),
    (12, 1, 136, ACT_SIGMOID, False, "none", True, 1, True),
    (6, 1, 136, ACT_GELU, True, "add", False, 1, True),
    (100, 1, 136, ACT_GELU, True, "dgelu", True, 1, True),
    (2, 130, 136, ACT_TANH, True, "none", True, 1, True),
    (6, 1, 136, ACT_NONE, False, "mask", False, 2, True),
    (12, 130, 136, ACT_TANH, False, "add", False, 1, True),
    (6, 130, 136, ACT_NONE, False, "mask", False, 1, False),
    (12, 1, 8, ACT_TANH, True, "none", False, 0, False),
    (100, 1, 8, ACT_TANH, False, "dgelu", False, 1, True),
    (2, 1, 136, ACT_TANH, True, "none", True, 1, False),
    (6, 130, 8, ACT_SIGMOID, False, "none", False, 0, True),
    (1, 130, 136, ACT_GELU, False, "none", False, 1, False),
    (1, 1, 8, ACT_GELU, False, "add", True, 1, True),
    (2, 1, 8, ACT_GELU, False, "none", True, 2, True),
    (2, 1, 136, ACT_NONE, False, "add", False, 0, True),
    (1, 1, 136, ACT_SIGMOID, True, "dgelu", False, 0, True),
    (100, 1, 136, ACT_TANH, False, "none", False, 2, True),
    (100, 1, 8, ACT_NONE, False, "mask", True, 2, False),
    (6, 130, 8, ACT_TANH, False, "add", False, 0, True),
    (2, 130, 136, ACT_TANH, False, "add", True, 1, True),
    (12, 130, 136, ACT_NONE, True, "none", True, 2, True),
    (1, 130, 136, ACT_TANH, False, "none", False, 0, False),
    (100, 130, 8, ACT_GELU, True, "dgelu", True, 0, False),
    (6, 130, 8, ACT_GELU, False, "add", True, 2, True),
    (6, 130, 8, ACT_GELU, True, "none", False, 0, True),
    (12, 1, 8, ACT_RELU, False, "mask", False, 1, True),
    (96, 1, 136, ACT_TANH, False, "add", True, 1, False),
    (200, 1, 8, ACT_GELU, True, "mask", False, 2, False),
    (200, 130, 136, ACT_RELU, False, "dgelu", False, 1, True),
    (200, 1, 136, ACT_RELU, False, "dgelu", True, 0, True),
    (96, 130, 8, ACT_TANH, True, "none", False, 2, False),
    (96, 130, 8, ACT_SIGMOID, True, "mask", True, 1, False),
    (96, 130, 8, ACT_SIGMOID, False, "none", False, 2, False),
    (200, 1, 8, ACT_SIGMOID, True, "mask", False, 2, False),
]


def build_narrow(combo, dtype, dev, idx):
    """-> (args, kw, allocations [C, C2 or None]): every [M, N] operand is a column slice inside a poisoned / sentinel allocation
    (8 columns either side: row strides stay multiples of 8 elements, so N alone decides which epilogue runs)"""
    N, M, K, act, has_bias, akind, has_aux2, c2, out_f32 = combo
    A = rnd((M, K), dtype, dev, 1100 + idx)
    W = rnd((N, K), dtype, dev, 2000 + idx, K ** -0.5)
    bias = rnd((N,), torch.float32, dev, 3300 + idx) if has_bias else None
    cbig, out = sentinel(M, N, torch.float32 if out_f32 else dtype, dev, 8, 8)
    kw = dict(out=out, act=act, c2_mode=c2, out_f32=out_f32)
    if akind != "none":
        _, kw["aux"] = poisoned(rnd((M, N), dtype, "cpu", 4400 + idx), dev, 8, 8)
        kw["mask_relu"], kw["mask_dgelu"] = akind == "mask", akind == "dgelu"
    if has_aux2:
        # +-(1 + N(0, 1/16)), signs in a chequerboard: never near zero, so that a dropped aux2 shows whatever the activation does
        # afterwards, and both signs reach the activation even in a single row
        sign = 1.0 - 2.0 * ((torch.arange(M).view(-1, 1) + torch.arange(N).view(1, -1)) % 2).float()
        _, kw["aux2"] = poisoned(((rnd((M, N), torch.float32, "cpu", 5000 + idx, 0.25) + 1.0) * sign).to(dtype), dev, 8, 8)
    c2big = None
    if c2:
        c2big, kw["out2"] = sentinel(M, N, dtype, dev, 8, 8)
    return (A, W, bias), kw, [cbig, c2big]


def build_classifier_head(B, N, dtype, dev):
    """the existence classifier's output layer: logits [B, K = 8] -> N in {1, 2} columns, bias, sigmoid, f32 output (compact, inside a
    sentinel allocation): -> (args, kw, allocation)"""
    A = rnd((B, 8), dtype, dev, 151)
    W = rnd((N, 8), dtype, dev, 152, 8 ** -0.5)
    bias = rnd((N,), torch.float32, dev, 153)
    big, out = sentinel(B, N, torch.float32, dev)
    return (A, W, bias), dict(out=out, act=ACT_SIGMOID, out_f32=True), big


# ---- TN gathers: (B, g, Nt, off, N, K); ways 1 .. 4
TN_CASES = [(9, 36, 37, 1, 64, 72), (21, 200, 201, 1, 136, 200), (60, 5, 6, 1, 8, 8)]
TN_WAYS = (1, 2, 3, 4)


def build_tn(case, way, dtype, dev):
    """-> (kw, compact kw, allocation around dW): ops.gemm_tn(**kw) with remapped / strided operands, and the same call on compact
    copies of the addressed rows.  dY carries M ** -0.5 (the reduction length, as B carries K ** -0.5 in the NT tests: results of
    unit scale, so the absolute part of the tolerance means the same).
      1: x_remap only (X = the poisoned token buffer);  2: dy_remap + dbias, X a column slice (ldx > K);  3: both remaps (+ dbias);
      4: way 2 accumulated onto prefilled dW / dbias."""
    B, g, Nt, off, N, K = case
    M = B * g
    s = M ** -0.5
    kw, ck = dict(M=M), dict()
    if way == 1:
        kw["dY"] = ck["dY"] = rnd((M, N), dtype, dev, 201, s)
    else:
        _, kw["dY"], ck["dY"] = token_rows(B, g, Nt, off, N, dtype, dev, 201, s)
        kw["dy_remap"] = (g, Nt, off)
    if way in (1, 3):
        _, kw["X"], ck["X"] = token_rows(B, g, Nt, off, K, dtype, dev, 202)
        kw["x_remap"] = (g, Nt, off)
    else:
        xc = rnd((M, K), dtype, "cpu", 202)
        _, kw["X"] = poisoned(xc, dev, 8, 16)
        ck["X"] = xc.to(dev)
    dbias = way != 1
    acc = way == 4
    big, dW = (poisoned(rnd((N, K), torch.float32, "cpu", 203), dev, 4, 4, fill=-1000.0) if acc else sentinel(N, K, torch.float32, dev, 4, 4))
    kw.update(dW=dW, accumulate=acc)
    ck.update(dW=dW.clone(), accumulate=acc)
    if dbias:
        db = rnd((N,), torch.float32, dev, 204) if acc else torch.full((N,), -1000.0, device=dev)
        kw["dbias"], ck["dbias"] = db, db.clone()
    return kw, ck, big


# ------------------------------------------------------------------------------------------------ a small call of a given form
def build_nt_of_form(f, dev, seed=300):
    """-> (args, kw for ops.gemm_nt / ops.gemm_nt_x3 (planes), reference args, reference kw for ref_gemm_nt) of a small problem whose
    signature is f: 3 images of 50 rows (two 128-row tiles, image ends inside a tile), N = 72, K = 64; a 2 x 7 x 9 x 64 map for the
    3x3 forms.  The plane calls need unmore_amd.ops to split their operands (GPU only)."""
    planes = f.kind == "planes"
    dtype = torch.bfloat16 if f.kind == "bf16" else torch.float32
    Bn, g, Nt, N, K = 3, 50, 51, 72, 64
    assert not (f.red or f.no_store), "the fused row reduction has its own tests (large shapes only)"
    if f.conv:
        nb, H, W, Cin = 2, 7, 9, 64
        s = 2 if f.conv == 2 else 1
        M = nb * ((H - 1) // s + 1) * ((W - 1) // s + 1)
        A = rnd((nb, H, W, Cin), dtype, dev, seed)
        Wt = rnd((N, 9 * Cin), dtype, dev, seed + 1, (9 * Cin) ** -0.5)
        Bn, g, Nt = 2, M // 2, M // 2 + 1
    else:
        M = Bn * g
        Wt = rnd((N, K), dtype, dev, seed + 1, K ** -0.5)
    kw = {}
    if not f.conv:
        if f.a_remap:
            _, A, _ = token_rows(Bn, g, Nt, 1, K, dtype, dev, seed)
            kw.update(M=M, a_remap=(g, Nt, 1))
        elif f.lda:
            _, A = poisoned(rnd((M, K), dtype, "cpu", seed), dev, 8, 8)
        else:
            A = rnd((M, K), dtype, dev, seed)
    bias = rnd((N,), torch.float32, dev, seed + 2) if f.bias else None
    if f.rowbias:
        kw.update(rowbias=rnd((Bn, N), torch.float32, dev, seed + 3), rows_per_batch=g)
    rows_c = Bn * Nt if f.c_remap else M
    if f.c_remap:
        kw["c_remap"] = (g, Nt, 1)
    odt = torch.float32 if (f.out_f32 or planes) else dtype
    out = None
    if f.alias:
        _, out = poisoned(rnd((rows_c, N), odt, "cpu", seed + 4), dev, 8 if f.ldc else 0, 8 if f.ldc else 0, fill=-1000.0)
    elif f.c_remap or f.ldc:
        _, out = sentinel(rows_c, N, odt, dev, 8 if f.ldc else 0, 8 if f.ldc else 0)
    if out is not None:
        kw["out"] = out
    a_t = None
    if f.aux != "none":
        if f.alias:
            a_t = out
        elif f.aux_mod:
            a_t = rnd((g, N), odt if planes else dtype, dev, seed + 5)
            kw["aux_mod"] = g
        else:
            a_t = rnd((rows_c, N), odt if planes else dtype, dev, seed + 5)
    if f.aux2:
        kw["aux2"] = rnd((rows_c, N), odt if planes else dtype, dev, seed + 6)
    kw.update(act=f.act, c2_mode=f.c2, conv=f.conv)
    rkw = dict(kw)
    if a_t is not None:
        rkw.update(aux=a_t, mask_relu=f.aux == "mask", mask_dgelu=f.aux == "dgelu")
    rkw["out_f32"] = f.out_f32 or planes
    if planes:
        if a_t is not None:
            kw[{"mask": "mask", "dgelu": "dgelu", "add": "aux"}[f.aux]] = a_t
        kw["out_planes"] = not f.out_f32
        return (A, Wt, bias), kw, (A, Wt, bias), rkw
    if a_t is not None:
        kw.update(aux=a_t, mask_relu=f.aux == "mask", mask_dgelu=f.aux == "dgelu")
    kw["out_f32"] = f.out_f32
    return (A, Wt, bias), kw, (A, Wt, bias), rkw


def build_tn_of_form(f, dev, seed=400):
    """-> (kw for ops.gemm_tn, reference kw for ref_gemm_tn) of a small problem whose signature is f (plane calls: the GPU test splits
    dY and X): 3 images of 50 rows, N = 72, K = 64; a 2 x 7 x 9 x 64 map for the 3x3 forms"""
    dtype = torch.bfloat16 if f.kind == "bf16" else torch.float32
    Bn, g, Nt, N, K = 3, 50, 51, 72, 64
    kw = {}
    if f.conv:
        nb, H, W, Cin = 2, 7, 9, 64
        s = 2 if f.conv == 2 else 1
        M = nb * ((H - 1) // s + 1) * ((W - 1) // s + 1)
        kw["X"] = rnd((nb, H, W, Cin), dtype, dev, seed)
        kw["conv"] = f.conv
        K = 9 * Cin
    else:
        M = Bn * g
        if f.x_remap:
            _, kw["X"], _ = token_rows(Bn, g, Nt, 1, K, dtype, dev, seed)
            kw["x_remap"] = (g, Nt, 1)
        elif f.ldx:
            _, kw["X"] = poisoned(rnd((M, K), dtype, "cpu", seed), dev, 8, 8)
        else:
            kw["X"] = rnd((M, K), dtype, dev, seed)
    sc = M ** -0.5
    if f.dy_remap:
        assert not f.conv
        _, kw["dY"], _ = token_rows(Bn, g, Nt, 1, N, dtype, dev, seed + 1, sc)
        kw["dy_remap"] = (g, Nt, 1)
    elif f.lddy:
        _, kw["dY"] = poisoned(rnd((M, N), dtype, "cpu", seed + 1, sc), dev, 8, 8)
    else:
        kw["dY"] = rnd((M, N), dtype, dev, seed + 1, sc)
    if f.dy_remap or f.x_remap:
        kw["M"] = M
    kw["dW"] = rnd((N, K), torch.float32, dev, seed + 2) if f.accumulate else torch.full((N, K), -1000.0, device=dev)
    kw["accumulate"] = f.accumulate
    if f.dbias:
        kw["dbias"] = rnd((N,), torch.float32, dev, seed + 3) if f.accumulate else torch.full((N,), -1000.0, device=dev)
    return kw


# ------------------------------------------------------------------------------------------------ which test pins which form
# Every form that one TrainStep.step on dpt_tiny (f32, bf16) and one prediction of the existence classifier launch
# (test_gemm_forms_gpu.py::test_every_engine_form_is_pinned records them), and the test that runs a call of exactly that signature
# against float64.  test_nt_engine_form / test_tn_engine_form build their call from the key itself (build_*_of_form).
# Fields: NTForm(kind, conv, act, aux, aux2, bias, rowbias, c2, out_f32, a_remap, c_remap, aux_mod, lda, ldc, alias, red, no_store),
#         TNForm(kind, conv, dbias, accumulate, dy_remap, x_remap, lddy, ldx)
_G = "test_gemm_forms_gpu.py::"
NT, TN, T, F_ = NTForm, TNForm, True, False
COVERED = {
    NT("bf16", 0, 0, "add", F_, F_, F_, 0, F_, F_, F_, F_, F_, T, T, F_, F_): _G + "test_nt_hook_grad_class_rows",
    NT("bf16", 0, 0, "add", F_, F_, F_, 0, F_, F_, T, F_, F_, F_, T, F_, F_): _G + "test_nt_hook_grad_token_rows",
    NT("bf16", 0, 0, "add", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 0, 0, "add", F_, T, F_, 0, F_, F_, T, T, F_, F_, F_, F_, F_): _G + "test_nt_patch_embed_form",
    NT("bf16", 0, 0, "dgelu", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_plain",
    NT("bf16", 0, 0, "mask", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 0, 0, "none", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 0, 0, "none", F_, F_, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 0, 0, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_plain",
    NT("bf16", 0, 0, "none", F_, T, F_, 0, T, F_, F_, F_, T, F_, F_, F_, F_): _G + "test_nt_readout_class_token_half",
    NT("bf16", 0, 1, "add", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 0, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 0, 2, "none", F_, F_, T, 2, F_, T, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_a_row_gather",
    NT("bf16", 0, 2, "none", F_, T, F_, 2, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_plain",
    NT("bf16", 0, 5, "none", F_, T, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_classifier_head_form",
    NT("bf16", 1, 0, "add", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 1, 0, "add", T, T, F_, 1, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 1, 0, "mask", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 1, 0, "mask", T, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 1, 0, "none", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 1, 0, "none", F_, F_, F_, 1, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 1, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("bf16", 2, 0, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_conv3x3_fwd",
    NT("bf16", 2, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 0, 0, "add", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, T, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 0, 0, "add", F_, F_, F_, 0, F_, F_, F_, F_, F_, T, T, F_, F_): _G + "test_nt_hook_grad_class_rows",
    NT("f32", 0, 0, "dgelu", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_plain",
    NT("f32", 0, 0, "none", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 0, 0, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_plain",
    NT("f32", 0, 0, "none", F_, T, F_, 0, T, F_, F_, F_, T, F_, F_, F_, F_): _G + "test_nt_readout_class_token_half",
    NT("f32", 0, 1, "add", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 0, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 0, 5, "none", F_, T, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_classifier_head_form",
    NT("f32", 1, 0, "none", F_, F_, F_, 1, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 1, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("f32", 2, 0, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_conv3x3_fwd",
    NT("f32", 2, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 0, "add", F_, F_, F_, 0, T, F_, T, F_, F_, F_, T, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 0, "add", F_, T, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 0, "add", F_, T, F_, 0, T, F_, T, T, F_, F_, F_, F_, F_): "test_x3_gpu.py::test_gemm_nt_x3_token_remap_and_broadcast_aux",
    NT("planes", 0, 0, "dgelu", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_x3_gpu.py::test_gemm_nt_x3_epilogues",
    NT("planes", 0, 0, "mask", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 0, "none", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 0, "none", F_, F_, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 0, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_x3_planes",
    NT("planes", 0, 0, "none", F_, T, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_x3_planes",
    NT("planes", 0, 1, "none", F_, T, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_nt_x3_planes",
    NT("planes", 0, 2, "none", F_, F_, T, 2, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 0, 2, "none", F_, T, F_, 2, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_x3_gpu.py::test_gemm_nt_x3_epilogues",
    NT("planes", 1, 0, "add", F_, T, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 0, "add", T, T, F_, 1, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 0, "mask", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_x3_gpu.py::test_conv3x3_x3_small_maps_split_k",
    NT("planes", 1, 0, "mask", F_, F_, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 0, "mask", T, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 0, "none", F_, F_, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 0, "none", F_, F_, F_, 0, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 0, "none", F_, F_, F_, 1, T, F_, F_, F_, F_, F_, F_, F_, F_): _G + "test_nt_engine_form",
    NT("planes", 1, 1, "none", F_, T, F_, 0, F_, F_, F_, F_, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_conv3x3_x3_planes",
    TN("bf16", 0, F_, F_, F_, F_, F_, T): _G + "test_tn_engine_form",
    TN("bf16", 0, F_, F_, F_, F_, T, F_): _G + "test_tn_engine_form",
    TN("bf16", 0, F_, F_, F_, T, F_, F_): _G + "test_tn_row_gathers",
    TN("bf16", 0, T, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_gemm_tn_plain",
    TN("bf16", 0, T, F_, F_, F_, T, F_): _G + "test_tn_engine_form",
    TN("bf16", 0, T, F_, T, F_, F_, F_): _G + "test_tn_engine_form",
    TN("bf16", 1, F_, F_, F_, F_, F_, F_): _G + "test_tn_engine_form",
    TN("bf16", 1, T, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_conv3x3_wgrad",
    TN("bf16", 2, T, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_conv3x3_wgrad",
    TN("f32", 0, F_, F_, F_, F_, F_, F_): _G + "test_tn_engine_form",
    TN("f32", 0, F_, F_, F_, F_, F_, T): _G + "test_tn_engine_form",
    TN("f32", 2, T, F_, F_, F_, F_, F_): "test_gemm_gpu.py::test_conv3x3_wgrad",
    TN("planes", 0, F_, F_, F_, F_, F_, F_): _G + "test_tn_engine_form",
    TN("planes", 0, T, F_, F_, F_, F_, F_): "test_x3_gpu.py::test_gemm_tn_x3_plain",
    TN("planes", 1, F_, F_, F_, F_, F_, F_): _G + "test_tn_engine_form",
    TN("planes", 1, T, F_, F_, F_, F_, F_): _G + "test_tn_engine_form",
}
