"""Every attention kernel (csrc/attention.hip) against the float64 reference of tests/attention_common.py under its row-wise bound
    ||got[r] - ref[r]||_2 <= c u ||A[r]||_2      (c from the CPU rounding model of the regime, never from a kernel's output: attention_common.C_OF)
through umr_attention_fwd / umr_attention_bwd themselves, on buffers with 64 sentinel elements either side and outputs pre-filled
with NaN (an element nobody wrote fails the bound).  The backward kernels get bf16(O_ref) and f32(lse_ref), so they are judged
independently of the forward kernel.  Every worst error / bound ratio is printed.

Sequence lengths (attention_common.NS):
    1, 2, 15, 16, 17    a partial first 16-row MFMA block
    63, 64, 65          the 64-key tile's edge; 64 skips the (N & 63) != 0 mask branch of the backward
    127                 the last N of the 16-queries-per-wave kernels and of the single-launch backward
    128                 the first of the 32-queries-per-wave kernels; an exact multiple, no mask
    129                 one query alone in the second workgroup
    191, 192, 193, 257  a slot of the two-deep LDS ring used a second (257: third) time; the last workgroup holds one query
(B, heads) = (3, 3) for N >= 64 and (2, 2) below: 18 / 27 workgroups at N >= 128, so the XCD map's remainder branch (nwg & 7 != 0)
runs, and grids below 8 at small N; every (b, h) has its own data, and batches b < B - 1 are followed by real data, not zeros.

Paths: bf16 forward <1> (N < 128) / <2>; f32 forward; bf16 backward in one launch (N < 128, UMR_ATTN_BWD_FUSED=1), in three launches
with <1> (N < 128, UMR_ATTN_BWD_FUSED=0: the only way to attn_bwd_dq_bf16_kernel<1> / attn_bwd_dkv_bf16_kernel<1>) and with <2>;
f32 backward.  The bit-equality tests compare the forward once per (dtype, N): under "unfused" only the backward is compared."""
import pytest
import torch

import attention_common as ac

pytestmark = pytest.mark.gpu
SENTINEL = 7680.0          # exact in bf16 and outside every value range used below
DTYPES = ["bf16", "f32"]
NAN = float("nan")

# (dtype, N, mode of the backward): "fused" / "unfused" set UMR_ATTN_BWD_FUSED to 1 / 0, "default" leaves it alone
BWD_CASES = [(dt, N, mode) for dt in DTYPES for N in ac.NS for mode in (("fused", "unfused") if dt == "bf16" and N < 128 else ("default",))]
BWD_IDS = [f"{dt}-N{N}-{mode}" for dt, N, mode in BWD_CASES]


def _L():
    from unmore_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(t, dtype, fill=SENTINEL):
    """a device copy of `t` with 64 sentinel elements before and after it in the same allocation -> (view, whole buffer)"""
    buf = torch.full((t.numel() + 128,), fill, dtype=dtype, device="cuda")
    view = buf[64:64 + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _guards_intact(*bufs):
    return all(bool((b[:64] == SENTINEL).all()) and bool((b[-64:] == SENTINEL).all()) for b in bufs)


def _bits(t):
    """the tensor's bit patterns, so that equality is bit equality (NaN included)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _set_mode(umr_opts, mode):
    if mode != "default":
        umr_opts.setenv("UMR_ATTN_BWD_FUSED", "1" if mode == "fused" else "0")


def _fwd(qkv, B, N, H, dtype, need_lse=True):
    """qkv: a guarded device view [B * N, 3 * H * 64] -> (out [B * N, H * 64], lse [B * H * N] or None), both device views"""
    L, td = _L(), ac.TORCH_DTYPE[dtype]
    out, obuf = _guarded(torch.full((B * N, H * ac.HD), NAN), td)
    lse, lbuf = _guarded(torch.full((B * H * N,), NAN), torch.float32) if need_lse else (None, None)
    L.check(L.lib().umr_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr() if need_lse else None, B, N, H, ac.HD,
                                      L.BF16 if dtype == "bf16" else L.F32, _stream()), "umr_attention_fwd")
    torch.cuda.synchronize()
    assert _guards_intact(obuf) and (lbuf is None or _guards_intact(lbuf)), "the forward wrote outside out / lse"
    return out, lse


def _bwd(qkv, out, dout, lse, B, N, H, dtype):
    """-> dqkv [B * N, 3 * H * 64], a device view; the dsum workspace has exactly the size umr_attention_bwd_workspace asks for"""
    L, td = _L(), ac.TORCH_DTYPE[dtype]
    dqkv, dbuf = _guarded(torch.full((B * N, 3 * H * ac.HD), NAN), td)
    nws = L.lib().umr_attention_bwd_workspace(B, N, H)
    assert nws == B * H * 2 * ((N + 63) // 64 * 64) * 4
    ws, wbuf = _guarded(torch.full((nws // 4,), NAN), torch.float32)
    L.check(L.lib().umr_attention_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), ws.data_ptr(), dqkv.data_ptr(), B, N, H,
                                      ac.HD, L.BF16 if dtype == "bf16" else L.F32, _stream()), "umr_attention_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(dbuf), "the backward wrote outside dqkv"
    assert _guards_intact(wbuf), "the backward wrote outside the dsum workspace"
    return dqkv


def _check(what, got, ref, dtype, regime):
    r = ac.ratios(got, ref, dtype, ac.C_OF[dtype][regime])
    print(f"attention bound | {what} | " + " ".join(f"{n} {v[0]:.4f}" for n, v in r.items()))
    over = {n: v for n, v in r.items() if v[1] != 0 or not v[0] <= 1.0}
    assert not over, f"{what}: (worst error / bound, rows over their bound) = {over}"


def _device_inputs(regime, N, dtype):
    """the regime's inputs in the kernels' layout on the device, each between guards: (qkv, dout, the buffers to check)"""
    i, td = ac.inputs(regime, N), ac.TORCH_DTYPE[dtype]
    qkv, qbuf = _guarded(ac.pack_qkv(i), td)
    dout, gbuf = _guarded(ac.pack_rows(i["dO"]), td)
    return qkv, dout, (qbuf, gbuf)


def _path(kind, dtype, N, mode="default"):
    if dtype == "f32":
        return f"{kind} f32"
    if kind == "fwd":
        return "fwd bf16 <1>" if N < 128 else "fwd bf16 <2>"
    return "bwd bf16 <2>" if N >= 128 else ("bwd bf16 one launch" if mode == "fused" else "bwd bf16 <1>")


@pytest.mark.parametrize("N", ac.NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_within_the_bound(dtype, N):
    """out and lse within the bound in every regime; without lse (a null pointer) the same bits in out"""
    B, H = ac.grid(N)
    for regime in ac.REGIMES:
        qkv, _, bufs = _device_inputs(regime, N, dtype)
        out, lse = _fwd(qkv, B, N, H, dtype)
        got = dict(O=ac.unpack_rows(out.cpu().double(), B, H, N), lse=lse.cpu().double().view(B, H, N))
        _check(f"{_path('fwd', dtype, N)} | N={N} {regime}", got, ac.ref_of(regime, N, dtype), dtype, regime)
        out2, _ = _fwd(qkv, B, N, H, dtype, need_lse=False)
        assert torch.equal(_bits(out2), _bits(out)), "out differs when lse is not asked for"
        assert _guards_intact(*bufs) and torch.equal(qkv.cpu().double(), ac.pack_qkv(ac.inputs(regime, N)))


@pytest.mark.parametrize("dtype,N,mode", BWD_CASES, ids=BWD_IDS)
def test_backward_within_the_bound(dtype, N, mode, umr_opts):
    """dQ, dK and dV, each against its own magnitude, in every regime, from the REFERENCE's O and lse rounded to the kernel's types"""
    B, H = ac.grid(N)
    _set_mode(umr_opts, mode)
    td = ac.TORCH_DTYPE[dtype]
    for regime in ac.REGIMES:
        ref = ac.ref_of(regime, N, dtype)
        qkv, dout, bufs = _device_inputs(regime, N, dtype)
        out, obuf = _guarded(ac.pack_rows(ref["O"]), td)
        lse, lbuf = _guarded(ref["lse"].reshape(-1), torch.float32)
        dqkv = _bwd(qkv, out, dout, lse, B, N, H, dtype)
        dQ, dK, dV = ac.unpack_dqkv(dqkv.cpu().double(), B, H, N)
        _check(f"{_path('bwd', dtype, N, mode)} | N={N} {regime}", dict(dQ=dQ, dK=dK, dV=dV), ref, dtype, regime)
        assert _guards_intact(obuf, lbuf, *bufs)


@pytest.mark.parametrize("dtype,N,mode", BWD_CASES, ids=BWD_IDS)
def test_each_slice_computes_what_it_computes_alone(dtype, N, mode, umr_opts):
    """The (B, heads) launch is BIT-identical to B * heads launches of one (b, h) slice as a B = 1, heads = 1 problem: forward, and
    backward chained on the device's own out and lse as the engine does.  A slice's arithmetic does not depend on where it lies --
    a workgroup's waves, lanes and tiles are the same in both launches -- only its addresses do: a difference is a stride, block-map
    or zero-fill error."""
    B, H = ac.grid(N)
    _set_mode(umr_opts, mode)
    td = ac.TORCH_DTYPE[dtype]
    for regime in ac.REGIMES:
        qkv, dout, bufs = _device_inputs(regime, N, dtype)
        out, lse = _fwd(qkv, B, N, H, dtype)
        dqkv = _bwd(qkv, out, dout, lse, B, N, H, dtype)
        assert bool(torch.isfinite(dqkv.float()).all())
        for b in range(B):
            for h in range(H):
                qkv1, q1buf = _guarded(qkv.view(B, N, 3, H, ac.HD)[b, :, :, h].reshape(N, 3 * ac.HD), td)
                dout1, g1buf = _guarded(dout.view(B, N, H, ac.HD)[b, :, h], td)
                out1, lse1 = _fwd(qkv1, 1, N, 1, dtype)
                dqkv1 = _bwd(qkv1, out1, dout1, lse1, 1, N, 1, dtype)
                where = f"{regime} N={N} slice (b={b}, h={h})"
                if mode != "unfused":          # (the same forward launches as under "fused")
                    assert torch.equal(_bits(out1), _bits(out.view(B, N, H, ac.HD)[b, :, h])), f"out, {where}"
                    assert torch.equal(_bits(lse1), _bits(lse.view(B, H, N)[b, h])), f"lse, {where}"
                assert torch.equal(_bits(dqkv1), _bits(dqkv.view(B, N, 3, H, ac.HD)[b, :, :, h].reshape(N, 3 * ac.HD))), f"dqkv, {where}"
                assert _guards_intact(q1buf, g1buf)
        assert _guards_intact(*bufs)


@pytest.mark.parametrize("dtype,N,mode", BWD_CASES, ids=BWD_IDS)
def test_two_runs_give_the_same_bits(dtype, N, mode, umr_opts):
    B, H = ac.grid(N)
    _set_mode(umr_opts, mode)
    for regime in ("diffuse", "rising"):
        qkv, dout, _ = _device_inputs(regime, N, dtype)
        runs = []
        for _ in range(2):
            out, lse = _fwd(qkv, B, N, H, dtype)
            runs.append((out, lse, _bwd(qkv, out, dout, lse, B, N, H, dtype)))
        for a, b in zip(*runs):
            assert torch.equal(_bits(a), _bits(b))
