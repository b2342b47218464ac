"""tests/attention_common.py checked on the CPU: the float64 reference against a hand-computed 3-key case, the constants of the bound
against the rounding model they are derived from, and the bound against five wrong variants of the reference -- the condition that keeps
it from being vacuous: a bound that every mutant passed would also pass a kernel with the mutant's defect.

Mutant figures (worst error / bound at c = 1, best of the five regimes; the assertion uses the WIDEST constant, C[dtype], for which
2 c = 9.3 in bf16 and 4896 in f32 -- every regime's own c is smaller):
  (a) last key never attended        bf16 >= 68 (dV, diffuse), far more elsewhere      f32 >= 2.2e6
  (b) zero rows join the softmax     bf16 >= 555 (lse, negative)                       f32 >= 3.6e6 (lse / O, negative)
      The four zero-mean regimes see many zero rows (diffuse: >= 95 with 47..63 of them) but not ONE (N = 63, 127, 191: 7.3, 3.7, 2.3 in
      bf16): a key of score 0 among N keys whose scores have zero mean weighs about 0.6 / N.  Where the real scores are negative
      on average it outweighs them, which is what the negative regime is for.
  (c) score scale off by 1 %         bf16 >= 314 (lse, sharp)                          f32 >= 1.9e6 (dV, sharp)
  (d) V rows 3 and 4 swapped         bf16 >= 699 (O, peaked / sharp)                   f32 >= 2.3e7
  (e) delta taken as zero            bf16 >= 146 (dQ / dK, peaked, sharp, rising)      f32 >= 4.8e6"""
import pytest
import torch

import attention_common as ac

DTYPES = ["bf16", "f32"]
NS_MUTANT = [N for N in ac.NS if N >= 17]


@pytest.fixture(scope="module")
def model_ratios():
    """{(dtype, regime, N): {output: worst error / bound at c = 1}} of the rounding model, computed once"""
    out = {}
    for dt in DTYPES:
        for reg in ac.REGIMES:
            for N in ac.NS:
                ref = ac.ref_of(reg, N, dt)
                r = ac.ratios(ac.MODEL[dt](ac.inputs(reg, N), ref), ref, dt, 1.0)
                out[(dt, reg, N)] = {n: v[0] for n, v in r.items()}
    return out


def test_reference_by_hand_three_keys():
    """q = e0 for three queries, k_j = 8 s_j e0 with s = (0, ln 2, 0): every row of P is (1/4, 1/2, 1/4) and lse = ln 4.
    v_j = a_j e1 with a = (4, 8, -4) and dO = e1: O = 4 e1, dP = a, delta = 4, dS = (0, 2, -2) per query."""
    ln2 = ac.LN2
    z = lambda: torch.zeros((3, 64), dtype=torch.float64)
    q, k, v, dO = z(), z(), z(), z()
    q[:, 0] = 1.0
    k[:, 0] = torch.tensor([0.0, 8 * ln2, 0.0], dtype=torch.float64)
    v[:, 1] = torch.tensor([4.0, 8.0, -4.0], dtype=torch.float64)
    dO[:, 1] = 1.0
    r = ac.reference(dict(q=q, k=k, v=v, dO=dO), "f32")
    e = lambda col, vals: torch.zeros((3, 64), dtype=torch.float64).index_put_((torch.arange(3), torch.full((3,), col)), torch.tensor(vals, dtype=torch.float64))
    close = lambda a, b: torch.testing.assert_close(a, b, atol=1e-14, rtol=1e-14)
    close(r["lse"], torch.full((3,), 2 * ln2, dtype=torch.float64))
    close(r["O"], e(1, [4.0, 4.0, 4.0]))
    close(r["dQ"], e(0, [2 * ln2] * 3))
    close(r["dK"], e(0, [0.0, 0.75, -0.75]))
    close(r["dV"], e(1, [0.75, 1.5, 0.75]))
    close(r["A_O"], e(1, [6.0, 6.0, 6.0]))
    close(r["A_dQ"], e(0, [6 * ln2] * 3))              # aS = P (|dP| + 4) = (2, 6, 2) per query
    close(r["A_dK"], e(0, [0.75, 2.25, 0.75]))
    close(r["A_dV"], e(1, [0.75, 1.5, 0.75]))
    # the bf16 path's operand rounding: 8 * 0.125 * log2 e = 1.4427 -> 185 / 128, so a key k = e0 scores 185 / 128 in log2 units
    assert ac.qhat(torch.tensor([8.0], dtype=torch.float64), "bf16").item() == 185.0 / 128.0
    q8, k1 = z(), z()
    q8[:, 0], k1[1, 0] = 8.0, 1.0
    rb = ac.reference(dict(q=q8, k=k1, v=v, dO=dO), "bf16")
    w = 2.0 ** (185.0 / 128.0)
    close(rb["lse"], torch.full((3,), 1.0, dtype=torch.float64) * torch.log(torch.tensor(2.0 + w, dtype=torch.float64)))
    close(rb["O"], e(1, [(4.0 + 8.0 * w - 4.0) / (2.0 + w)] * 3))


def test_inputs_are_bf16_values_distinct_per_slice_and_survive_the_layout():
    for reg in ac.REGIMES:
        i = ac.inputs(reg, 65)
        B, H = ac.grid(65)
        assert (B, H) == (3, 3) and ac.grid(63) == (2, 2)
        for n in ("q", "k", "v", "dO"):
            t = i[n]
            assert t.shape == (B, H, 65, 64) and torch.equal(t, ac.bf16r(t))
            flat = t.reshape(B * H, -1)
            assert all(not torch.equal(flat[a], flat[b]) for a in range(B * H) for b in range(a))
        dq, dk, dv = ac.unpack_dqkv(ac.pack_qkv(i), B, H, 65)
        assert torch.equal(dq, i["q"]) and torch.equal(dk, i["k"]) and torch.equal(dv, i["v"])
        assert torch.equal(ac.unpack_rows(ac.pack_rows(i["dO"]), B, H, 65), i["dO"])
    qkv = ac.pack_qkv(ac.inputs("diffuse", 2))          # [B * N, 3 * heads * 64]: token (b, n), then q | k | v, then the head
    assert torch.equal(qkv[1 * 2 + 1, 1 * 128 + 1 * 64:1 * 128 + 2 * 64], ac.inputs("diffuse", 2)["k"][1, 1, 1])


def test_worst_ratio_counts_rows_and_fails_nan_and_zero_bounds():
    err = torch.tensor([0.5, 2.0, 0.0, 1e-30], dtype=torch.float64)
    bnd = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64)
    assert ac.worst_ratio(err[:3], bnd[:3]) == (2.0, 1)
    assert ac.worst_ratio(err, bnd) == (float("inf"), 2)
    ref = dict(O=torch.zeros((2, 64), dtype=torch.float64), A_O=torch.ones((2, 64), dtype=torch.float64))
    got = torch.zeros((2, 64))
    got[1, 5] = float("nan")
    assert ac.ratios(dict(O=got), ref, "bf16", 1.0)["O"] == (float("inf"), 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_constants_are_what_the_model_measures(dtype, model_ratios):
    worst = {n: max(r[n] for (dt, _, _), r in model_ratios.items() if dt == dtype) for n in ac.OUTPUTS}
    print(f"{dtype}: model's worst row ratios {({n: round(v, 4) for n, v in worst.items()})}, c = {ac.C[dtype]}")
    for n in ac.OUTPUTS:
        assert 0.97 * ac.MODEL_WORST[dtype][n] <= worst[n] <= ac.MODEL_WORST[dtype][n], (n, worst[n])
    assert ac.C[dtype] == ac.SAFETY[dtype] * max(ac.MODEL_WORST[dtype].values())
    assert set(ac.MODEL_WORST_REGIME[dtype]) == set(ac.REGIMES)
    for reg in ac.REGIMES:
        w = max(max(r.values()) for (dt, g, _), r in model_ratios.items() if dt == dtype and g == reg)
        print(f"{dtype} {reg}: model's worst row ratio {w:.4f}, c = {ac.C_OF[dtype][reg]}")
        assert 0.97 * ac.MODEL_WORST_REGIME[dtype][reg] <= w <= ac.MODEL_WORST_REGIME[dtype][reg], (reg, w)
        assert ac.C_OF[dtype][reg] == ac.SAFETY[dtype] * ac.MODEL_WORST_REGIME[dtype][reg] <= ac.C[dtype]
    assert ac.SAFETY == {"bf16": 2.0, "f32": 4.0}


@pytest.mark.parametrize("N", ac.NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rounding_model_stays_below_half_the_bound(dtype, N, model_ratios):
    for reg in ac.REGIMES:
        r = {n: v / ac.C_OF[dtype][reg] for n, v in model_ratios[(dtype, reg, N)].items()}
        print(f"{dtype} N={N} {reg}: model error / bound " + " ".join(f"{n} {v:.3f}" for n, v in r.items()))
        assert set(r) == set(ac.OUTPUTS) and max(r.values()) <= 0.5, (reg, r)


MUTANT_CASES = [(m, N) for m in ac.MUTANTS for N in NS_MUTANT if not (m == "b" and N % 64 == 0)]     # (b): no zero rows at a multiple of 64


@pytest.mark.parametrize("mutant,N", MUTANT_CASES, ids=[f"{m}-N{N}" for m, N in MUTANT_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_mutant_is_over_twice_the_bound_in_some_regime(dtype, mutant, N):
    """against the widest constant of the dtype: what exceeds 2 C[dtype] exceeds twice every regime's own bound"""
    best = 0.0
    for reg in ac.REGIMES:
        r = ac.ratios(ac.reference(ac.inputs(reg, N), dtype, mutant), ac.ref_of(reg, N, dtype), dtype, ac.C[dtype])
        n, (ratio, bad) = max(r.items(), key=lambda kv: kv[1][0])
        print(f"{dtype} ({mutant}) N={N} {reg}: worst error / bound {ratio:.2f} on {n}, {bad} rows over")
        best = max(best, ratio)
    assert best > 2.0, f"({mutant}) {ac.MUTANTS[mutant]}: at most {best:.2f} x the bound at N = {N}"


@pytest.mark.parametrize("N", [129, 193, 257])
def test_rising_regime_crosses_the_deferral_threshold_both_ways(N):
    """the bf16 forward raises its running maximum only when a 64-key tile tops it by more than 8 log2 units: in the rising regime
    some (query, tile) pairs must take that branch and others must top the maximum by less and leave it stale"""
    i = ac.inputs("rising", N)
    s2 = ac.qhat(i["q"], "bf16") @ i["k"].transpose(-1, -2)                   # log2 units
    tiles = [s2[..., j:j + 64].max(-1).values for j in range(0, N, 64)]
    m, raised, stale = tiles[0].clone(), 0, 0
    for t in tiles[1:]:
        rel = t - m
        raised += int((rel > 8).sum())
        stale += int(((rel > 0) & (rel <= 8)).sum())
        m = torch.where(rel > 8, t, m)
    assert raised >= 100 and stale >= 100, (raised, stale)
