"""Plain float64 restatement of the attention kernels (csrc/attention.hip), the row-wise error bound they are held to, the rounding
model the bound's constant comes from, and float64 mutants that show the bound is not vacuous.  torch on the CPU only.

One (batch, head) slice is q, k, v, dO of shape [N, 64]; every function below works on [..., N, 64] (the tests pass [B, heads, N, 64]).
All inputs are bf16-representable, so the bf16 and the f32 kernels read the same numbers.

Reference (float64):
    bf16 path: q^ = bf16(f32(q) * (0.125f * 1.4426950408889634f)) -- the ONE operand rounding the bf16 kernels document and share
               (the forward kernel's comment on Q, the dQ body, the dK / dV body's in-place rescale of the Q tile);
    f32 path:  q^ = q * 0.125 * log2 e, unrounded
    S = q^ k^T ln 2,  P = softmax(S),  O = P v,  lse = logsumexp(S)
    dP = dO v^T,  delta = rowsum(dO o O),  dS = P o (dP - delta)
    dQ = 0.125 dS k,  dK = 0.125 dS^T q,  dV = P^T dO
Magnitudes (the same sums over absolute values, as S of linear_head_common.py):
    A_O = P |v|,  aS = P o (|dP| + rowsum(|dO| o |O|)),  A_dQ = 0.125 aS |k|,  A_dK = 0.125 aS^T |q|,  A_dV = P^T |dO|
Criterion, for every row r of every output (query rows of O and dQ, key rows of dK and dV):
    ||got[r] - ref[r]||_2 <= c u ||A[r]||_2,           u = 2^-9 (bf16), 2^-24 (f32)
    |lse_got - lse_ref|   <= c u + 4 * 2^-24 * max(1, |lse_ref|)

c is NOT tuned on a kernel's output.  It comes from a rounding model evaluated on the CPU over every input of the device test:
    bf16: float64 arithmetic, rounded to bf16 exactly where the kernels round: q^, the unnormalised P before P v and before the row sum l,
          the stored O, dS, P before P^T dO, q^ as the operand of dK (the kernel forms dK = ln 2 * dS^T q^), and the stored gradients;
          delta is taken from the bf16 O and the probabilities of the backward from the f32 lse, which is what the device test feeds.
          c = 2 x the model's worst row ratio; the factor 2 is for what the model leaves out: the order of f32 accumulation, the
          hardware exp2, and probabilities held relative to a running maximum that may be up to 2^8 stale (DEFER in the kernel).
    f32:  the reference's formulas evaluated in torch.float32; c = 4 x the worst row ratio (summation order differs more).
The recipe is applied per regime (C_OF): a regime's c is 2 x (4 x) the model's worst ratio over that regime's own inputs, which is never
more than the single constant over all inputs (C) and much less where the scores are small.
tests/test_attention_bound_cpu.py measures all of them and requires the constants below to be what it measures."""
import functools

import torch

HD = 64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
U = {"bf16": 2.0 ** -9, "f32": 2.0 ** -24}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}

# sequence lengths of the device test (tests/test_attention_bound_gpu.py says what each one reaches)
NS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]
REGIMES = ["diffuse", "peaked", "sharp", "rising", "negative"]
OUTPUTS = ["O", "lse", "dQ", "dK", "dV"]
MUTANTS = {
    "a": "the last key is never attended",
    "b": "the zero key / value rows up to the next multiple of 64 join the softmax",
    "c": "the score scale is off by 1 %",
    "d": "the V rows of keys 3 and 4 are swapped",
    "e": "delta is taken as zero",
}

# Worst row ratio error / (u ||A||) of the rounding model over all NS and all (b, h), as measured by
# test_attention_bound_cpu.py::test_constants_are_what_the_model_measures (which fails if these drift from what it computes); rounded up
# to three digits.  Per output over all regimes:
MODEL_WORST = {      # measured bf16 1.2363 0.8762 0.5671 1.3564 2.3162 (sharp, except dQ: rising); f32 169.58 7.325 56.72 111.99 611.99 (sharp)
    "bf16": {"O": 1.24, "lse": 0.877, "dQ": 0.568, "dK": 1.36, "dV": 2.32},
    "f32": {"O": 170.0, "lse": 7.33, "dQ": 56.8, "dK": 112.0, "dV": 612.0},
}
# ... and per regime over all outputs.  In f32 the relative error of a probability is about 2^-24 |S|, so the model's ratio follows the
# size of the scores: 7.5 where they are O(1), 612 where they reach +-100.
MODEL_WORST_REGIME = {
    "bf16": {"diffuse": 1.36, "peaked": 2.09, "sharp": 2.32, "rising": 2.04, "negative": 1.38},
    "f32": {"diffuse": 7.49, "peaked": 121.0, "sharp": 612.0, "rising": 76.1, "negative": 15.8},
}
SAFETY = {"bf16": 2.0, "f32": 4.0}
# c as the recipe gives it, one per dtype: bf16 4.64, f32 2448 ...
C = {d: SAFETY[d] * max(MODEL_WORST[d].values()) for d in U}
# ... and the c every check uses: the same recipe applied to each regime's own inputs, never larger than C[dtype].  One constant per dtype
# would hold the f32 kernels in diffuse to a bound 80 times wider than their own model's.
C_OF = {d: {r: SAFETY[d] * w for r, w in MODEL_WORST_REGIME[d].items()} for d in U}


def grid(N):
    """(B, heads) of the device test: 18 / 27 workgroups at N >= 128 (the XCD map's remainder branch), fewer than 8 at small N"""
    return (3, 3) if N >= 64 else (2, 2)


def bf16r(x):
    """float64 -> f32 -> bf16 (round to nearest even, as the kernels' casts) -> float64"""
    return x.float().bfloat16().double()


@functools.lru_cache(maxsize=None)
def inputs(regime, N):
    """q, k, v, dO [B, heads, N, 64] float64 holding bf16 values; a distinct seed per (regime, N, b, h).  Shared, never modified.
    diffuse: randn -- hundreds of near-equal scores: sensitive to mask and normalisation errors
    peaked:  q, k x 2.4
    sharp:   q, k x 4 -- a few keys per query carry everything: sensitive to key / value indexing and to the scale
    rising:  q x 2, key norms ramp 0.5 -> 3 along the sequence: the running maximum rises by less and by more than the kernel's
             8-log2-unit deferral threshold from tile to tile (test_attention_bound_cpu.py counts both events)
    negative: q + 0.75, k - 0.75 -- every score about -4.5 on average, so a zero-filled key that joins the softmax outweighs the real
             ones: the regime that sees ONE such key (N % 64 == 63) under the bf16 bound, which the zero-mean regimes cannot"""
    B, H = grid(N)
    out = torch.empty((4, B, H, N, HD), dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            g = torch.Generator().manual_seed(((REGIMES.index(regime) * 1000 + N) * 8 + b) * 8 + h)
            t = torch.randn((4, N, HD), generator=g)
            if regime == "peaked":
                t[:2] *= 2.4
            elif regime == "sharp":
                t[:2] *= 4.0
            elif regime == "rising":
                t[0] *= 2.0
                t[1] *= torch.linspace(0.5, 3.0, N)[:, None]
            elif regime == "negative":
                t[0] += 0.75
                t[1] -= 0.75
            out[:, b, h] = t.bfloat16().double()
    return dict(q=out[0], k=out[1], v=out[2], dO=out[3])


def qhat(q, dtype):
    if dtype == "bf16":
        scale = torch.tensor(LOG2E, dtype=torch.float32) * 0.125          # 0.125f * 1.4426950408889634f
        return (q.float() * scale).bfloat16().double()
    return q * (0.125 * LOG2E)


def reference(i, dtype, mutant=None):
    """float64 -> dict of O, lse, dQ, dK, dV and the magnitudes A_O, A_dQ, A_dK, A_dV.  `mutant`: one of MUTANTS, a deliberately wrong
    variant (CPU test only)"""
    q, k, v, dO = i["q"], i["k"], i["v"], i["dO"]
    N = q.shape[-2]
    kk, vv = k, v
    if mutant == "b":
        pad = torch.zeros(q.shape[:-2] + ((-N) % 64, HD), dtype=torch.float64)
        kk, vv = torch.cat([k, pad], -2), torch.cat([v, pad], -2)
    if mutant == "d":
        vv = v.clone()
        vv[..., 3, :], vv[..., 4, :] = v[..., 4, :], v[..., 3, :]
    S = qhat(q, dtype) @ kk.transpose(-1, -2) * LN2
    if mutant == "a":
        S[..., -1] = float("-inf")
    if mutant == "c":
        S = S * 1.01
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ vv
    dP = dO @ vv.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    if mutant == "e":
        delta = torch.zeros_like(delta)
    dS = P * (dP - delta)
    aS = P * (dP.abs() + (dO.abs() * O.abs()).sum(-1, keepdim=True))
    r = dict(O=O, lse=lse, dQ=0.125 * dS @ kk, dK=(0.125 * dS.transpose(-1, -2) @ q)[..., :N, :], dV=(P.transpose(-1, -2) @ dO)[..., :N, :])
    if mutant is None:
        r.update(A_O=P @ v.abs(), A_dQ=0.125 * aS @ k.abs(), A_dK=0.125 * aS.transpose(-1, -2) @ q.abs(), A_dV=P.transpose(-1, -2) @ dO.abs())
    return r


@functools.lru_cache(maxsize=None)
def ref_of(regime, N, dtype):
    """the reference of one input set, computed once and shared by every test that needs it (never modified)"""
    return reference(inputs(regime, N), dtype)


def model_bf16(i, ref):
    """float64 with the bf16 kernels' roundings.  The backward starts from bf16(ref O) and f32(ref lse), as the device test does."""
    q, k, v, dO = i["q"], i["k"], i["v"], i["dO"]
    qh = qhat(q, "bf16")
    S = qh @ k.transpose(-1, -2) * LN2
    m = S.max(-1, keepdim=True).values
    p = bf16r(torch.exp(S - m))                                   # the numerator AND the row sum use the rounded probabilities
    l = p.sum(-1, keepdim=True)
    O = bf16r(p @ v / l)
    lse = (m + torch.log(l))[..., 0].float().double()
    P = torch.exp(S - ref["lse"].float().double()[..., None])
    delta = (dO * bf16r(ref["O"])).sum(-1, keepdim=True)
    dS = bf16r(P * (dO @ v.transpose(-1, -2) - delta))
    return dict(O=O, lse=lse, dQ=bf16r(0.125 * dS @ k), dK=bf16r(LN2 * dS.transpose(-1, -2) @ qh), dV=bf16r(bf16r(P).transpose(-1, -2) @ dO))


def _mm32(a, b):
    """a [..., M, K] @ b [..., K, L] in f32, one product and one addition per term in the order of k: IEEE operations only, so the
    model's figures do not depend on the BLAS, the thread count or the vector width of the machine that runs the test"""
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
    for kk in range(a.shape[-1]):
        acc = acc + a[..., :, kk:kk + 1] * b[..., kk:kk + 1, :]
    return acc


def _rowsum32(x):
    return _mm32(x, torch.ones(x.shape[:-2] + (x.shape[-1], 1), dtype=torch.float32))


def model_f32(i, ref):
    """the reference's formulas in torch.float32 (sums in sequential order, see _mm32).  The backward starts from f32(ref O) and
    f32(ref lse), as the device test does."""
    q, k, v, dO = (i[n].float() for n in ("q", "k", "v", "dO"))
    T = lambda t: t.transpose(-1, -2)
    qh = q * (torch.tensor(LOG2E, dtype=torch.float32) * 0.125)
    S = _mm32(qh, T(k)) * torch.tensor(LN2, dtype=torch.float32)
    m = S.max(-1, keepdim=True).values
    p = torch.exp(S - m)
    l = _rowsum32(p)
    O = _mm32(p, v) / l
    lse = (m + torch.log(l))[..., 0]
    P = torch.exp(S - ref["lse"].float()[..., None])
    delta = _rowsum32(dO * ref["O"].float())
    dS = P * (_mm32(dO, T(v)) - delta)
    out = dict(O=O, lse=lse, dQ=0.125 * _mm32(dS, k), dK=0.125 * _mm32(T(dS), q), dV=_mm32(T(P), dO))
    assert all(t.dtype == torch.float32 for t in out.values())
    return {n: t.double() for n, t in out.items()}


MODEL = {"bf16": model_bf16, "f32": model_f32}


def bound(ref, name, dtype, c):
    """the bound of output `name` with constant c: per row [..., N]"""
    if name == "lse":
        return c * U[dtype] + 4 * 2.0 ** -24 * ref["lse"].abs().clamp(min=1.0)
    return c * U[dtype] * ref["A_" + name].norm(dim=-1)


def row_error(got, ref, name):
    d = got.double() - ref[name]
    err = d.abs() if name == "lse" else d.norm(dim=-1)
    return torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))     # an unwritten (NaN) element fails


def worst_ratio(err, bnd):
    """-> (the largest error / bound over the rows, the number of rows over their bound); a row whose bound is 0 must be exact"""
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()), int((ratio > 1).sum())


def ratios(got, ref, dtype, c):
    """{output name: (worst error / bound, rows over)} for every output present in `got`"""
    return {n: worst_ratio(row_error(got[n], ref, n), bound(ref, n, dtype, c)) for n in OUTPUTS if n in got}


# ---------------------------------------------------------------------------------------------- the kernels' memory layout
def pack_qkv(i):
    """q, k, v [B, heads, N, 64] -> the qkv-GEMM output [B * N, 3 * heads * 64] (q | k | v, heads contiguous inside each)"""
    B, H, N, _ = i["q"].shape
    return torch.stack([i["q"], i["k"], i["v"]], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * HD).contiguous()


def pack_rows(t):
    """[B, heads, N, 64] -> [B * N, heads * 64] (out, dout)"""
    B, H, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * HD).contiguous()


def unpack_rows(t, B, H, N):
    return t.reshape(B, N, H, HD).permute(0, 2, 1, 3)


def unpack_dqkv(t, B, H, N):
    """[B * N, 3 * heads * 64] -> dQ, dK, dV [B, heads, N, 64]"""
    x = t.reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]
