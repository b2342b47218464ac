"""The kernels of the collapsed boundary-distance head (csrc/linear_head.hip) and the small streaming helpers of the same train step
(csrc/elementwise.hip: segsum, fill_cls, cast, scale_by_device_scalar), each called directly through its ops wrapper and compared with
the plain float64 restatement of tests/linear_head_common.py (itself checked against conv2d / autograd in test_head_kernels_cpu.py).

Two kinds of input:
 (a) integer-valued: x in -3..3, weights / biases / dout in -2..2, prior dx in -8..8, act none.  Every partial sum in any order is an
     integer below 2^24 (asserted on the reference's S = sum |terms|), so f32 accumulation is exact and the device result must EQUAL
     the restatement: a pixel, tap, channel, run or slab that is skipped, doubled or shifted changes an integer.
 (b) randn with tanh / none / sine (forward): |out - ref| <= n * 2^-24 * S, the order-independent worst case of f32 summation of n
     terms (linear_head_common's docstring says what a term is), + 2^-21 behind tanhf / sinf (above the 5 ulp of OpenCL's full
     profile; the build passes no fast-math flag), + half a bf16 ulp of the reference for a bf16 result.  n <= 16384 keeps the bound
     below 2^-10 relative to S, which accumulation in bf16 would exceed.  The worst error / bound ratio is printed, not asserted.

Shapes: the backward kernels work in runs of up to 64 pixels of one row with a by-4 blocked loop and a remainder loop, so the widths
are 1, 2, 3, 5 (one short run), 63 (remainder 3), 64, 65 / 130 (a last run of width 1 / 2), 66, 67 (remainders 2, 3); the heights
include single rows; B >= 2 with different images, so a row test that let row -1 be the previous image's last row would show."""
import functools
import re
import time

import pytest
import torch

import linear_head_common as lh

pytestmark = pytest.mark.gpu
C = 256
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
SENTINEL = 7680.0          # exact in bf16 and outside every value range used below


def _ops():
    from unmore_amd import ops
    return ops


def _ints(shape, m, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-m, m + 1, shape, generator=g, device=device).float()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _guarded(t, dtype=None, fill=SENTINEL):
    """a device copy of `t` with 64 sentinel elements before and after it in the same allocation -> (view, whole buffer)"""
    dtype = dtype or t.dtype
    buf = torch.full((t.numel() + 128,), fill, dtype=dtype, device="cuda")
    view = buf[64:64 + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _guards_intact(buf, fill=SENTINEL):
    return bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all())


# ---------------------------------------------------------------------------------------------- linear head, kind (a)
# (B, H, W): property
INT_SHAPES = [
    ((2, 1, 1), "1x1 images: only the centre tap is inside"),
    ((2, 1, 2), "single row, width 2"),
    ((3, 1, 67), "single row: full run + ragged run of 3"),
    ((2, 2, 1), "single column, two rows"),
    ((2, 2, 5), "one run of 5: main loop once, remainder 1"),
    ((2, 2, 65), "last run of width 1"),
    ((2, 3, 1), "single column"),
    ((2, 3, 2), "run of 2: remainder loop only"),
    ((2, 3, 3), "run of 3: remainder loop only"),
    ((2, 3, 5), "remainder 1"),
    ((2, 3, 63), "one run, remainder 3"),
    ((2, 3, 64), "exactly one full run"),
    ((2, 3, 65), "full run + run of 1"),
    ((2, 3, 66), "full run + run of 2"),
    ((2, 3, 67), "full run + run of 3"),
    ((2, 3, 130), "two full runs + run of 2"),
    ((3, 7, 1), "single column, 7 rows, three images"),
    ((2, 7, 3), "7 rows of one run of 3"),
    ((2, 7, 130), "42 runs: bwd_weight with M <= 4096 -> one block"),
    ((1, 67, 130), "201 runs over 3 blocks of 67 runs (not a multiple of 4: unequal waves)"),
]
INT_IDS = ["B%dxH%dxW%d" % s for s, _ in INT_SHAPES]
INT_PARAMS = [s for s, _ in INT_SHAPES]


@functools.lru_cache(maxsize=None)
def _int_inputs(B, H, W):
    seed = (B * 1000 + H) * 1000 + W
    return dict(x=_ints((B, H, W, C), 3, seed), kw=_ints((9, C), 2, seed + 1), tb=_ints((10,), 2, seed + 2), dout=_ints((B, 1, H, W), 2, seed + 3),
                prior=_ints((B, H, W, C), 8, seed + 4), junk=_randn((B, 1, H, W), seed + 5))


@functools.lru_cache(maxsize=None)
def _int_ref(kind, B, H, W):
    """the float64 reference of one kernel at one shape, computed once and shared by the dtype / accumulate cases (never modified)"""
    i = _int_inputs(B, H, W)
    if kind == "fwd":
        out, S, _ = lh.fwd(i["x"], i["kw"], i["tb"], lh.ACT_NONE)
    elif kind == "data":
        out, S, _ = lh.bwd_data(i["dout"], None, i["kw"], lh.ACT_NONE)
    elif kind == "data_acc":
        out, S, _ = lh.bwd_data(i["dout"], None, i["kw"], lh.ACT_NONE, prior=i["prior"])
    else:
        out, S, _ = lh.bwd_weight(i["x"], i["dout"], None, lh.ACT_NONE)
    assert S.max().item() < 2 ** 24          # every partial sum is an integer f32 holds: equality is legitimate
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", INT_PARAMS, ids=INT_IDS)
def test_linear_head_fwd_exact(B, H, W, dtype):
    i = _int_inputs(B, H, W)
    out = _ops().linear_head_fwd(i["x"].to(dtype).cuda(), i["kw"].cuda(), i["tb"].cuda(), lh.ACT_NONE)
    assert out.shape == (B, 1, H, W) and out.dtype == torch.float32
    assert torch.equal(out.cpu().double(), _int_ref("fwd", B, H, W))


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", INT_PARAMS, ids=INT_IDS)
def test_linear_head_bwd_data_exact(B, H, W, dtype, accumulate):
    """overwrite: dx is pre-filled with NaN, every element must be written and none read; accumulate: onto non-zero contents.
    act none ignores yout: f32 passes None, bf16 passes a map of junk that must not be read into the result"""
    i = _int_inputs(B, H, W)
    start = i["prior"] if accumulate else torch.full((B, H, W, C), float("nan"))
    dx, buf = _guarded(start, dtype)
    yout = None if dtype == torch.float32 else i["junk"].cuda()
    ret = _ops().linear_head_bwd_data(i["dout"].cuda(), yout, i["kw"].cuda(), dx, lh.ACT_NONE, accumulate)
    assert ret.data_ptr() == dx.data_ptr()
    assert torch.equal(dx.cpu().double(), _int_ref("data_acc" if accumulate else "data", B, H, W))     # bf16: |value| <= 9*3*2 + 8 < 256, exact
    assert _guards_intact(buf)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", INT_PARAMS, ids=INT_IDS)
def test_linear_head_bwd_weight_exact(B, H, W, dtype):
    i = _int_inputs(B, H, W)
    yout = None if dtype == torch.float32 else i["junk"].cuda()
    R = _ops().linear_head_bwd_weight(i["x"].to(dtype).cuda(), i["dout"].cuda(), yout, lh.ACT_NONE)
    ref = _int_ref("weight", B, H, W)
    assert R.shape == (9 * C + 10,) and R.dtype == torch.float32
    got = R.cpu().double()
    assert torch.equal(got[9 * C:], ref[9 * C:]), "n[0..8], D"
    assert torch.equal(got[:9 * C], ref[:9 * C]), "G"


# ------------------------------------------------------------------------- linear head, kind (a): the launch plans of large inputs
def test_linear_head_fwd_exact_past_the_grid_cap():
    """M = 66600 pixels > 4 * 16384: the grid-stride loop of lh_fwd_kernel takes a second trip; W = 3 keeps x at 68 MB"""
    B, H, W = 3, 7400, 3
    assert B * H * W > 4 * 16384
    x, kw, tb = _ints((B, H, W, C), 3, 11, "cuda"), _ints((9, C), 2, 12), _ints((10,), 2, 13)
    out = _ops().linear_head_fwd(x, kw.cuda(), tb.cuda(), lh.ACT_NONE)
    ref, S, _ = lh.fwd(x, kw.cuda(), tb.cuda(), lh.ACT_NONE)           # float64 on the device
    assert S.max().item() < 2 ** 24
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_linear_head_bwd_data_exact_past_the_grid_cap(accumulate):
    """33000 runs > 4 * 8192: the grid-stride loop of lh_bwd_data_kernel takes a second trip; W = 1 keeps dx at 34 MB"""
    B, H, W = 11, 3000, 1
    assert B * H * ((W + 63) // 64) > 4 * 8192
    dout, kw = _ints((B, 1, H, W), 2, 21, "cuda"), _ints((9, C), 2, 22).cuda()
    prior = _ints((B, H, W, C), 8, 23, "cuda")
    dx, buf = _guarded(prior if accumulate else torch.full((B, H, W, C), float("nan")))
    _ops().linear_head_bwd_data(dout, None, kw, dx, lh.ACT_NONE, accumulate)
    ref, S, _ = lh.bwd_data(dout, None, kw, lh.ACT_NONE, prior=prior if accumulate else None)
    assert S.max().item() < 2 ** 24
    assert torch.equal(dx.double(), ref) and _guards_intact(buf)


def test_linear_head_bwd_weight_exact_on_the_production_reduce_path():
    """B = 2, H = 360, W = 640, bf16: M = 460800 -> 113 partial slabs, so lh_reduce_kernel's phase 0 takes the 8-way unrolled loop
    (slabs 0, 16, .. 112) and phases 1..15 the tail loop, over all 37 column blocks; 7200 runs in blocks of 64, the last block 32.
    The reference is formed on the device in float64, one image at a time."""
    B, H, W = 2, 360, 640
    assert (B * H * W + 4095) // 4096 == 113
    x = _ints((B, H, W, C), 3, 31, "cuda").to(torch.bfloat16)
    dout = _ints((B, 1, H, W), 2, 32, "cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    R = _ops().linear_head_bwd_weight(x, dout, None, lh.ACT_NONE)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ref, S, _ = lh.bwd_weight(x, dout, None, lh.ACT_NONE)
    smax = S.max().item()
    t2 = time.perf_counter()
    print(f"bwd_weight B{B} H{H} W{W} bf16: kernel call {1e3 * (t1 - t0):.1f} ms, float64 reference {t2 - t1:.2f} s, max S = {smax:.0f}")
    assert smax < 2 ** 24
    got = R.double()
    assert torch.equal(got[9 * C:], ref[9 * C:]), "n[0..8], D"
    assert torch.equal(got[:9 * C], ref[:9 * C]), "G"


# ---------------------------------------------------------------------------------------------- linear head, kind (b)
# at most four small shapes (M <= 4096); every tap with any term has at least 3 (linear_head_common's docstring): H, W in {1} or >= 4,
# or both >= 3
REAL_SHAPES = [(2, 3, 5), (2, 1, 67), (2, 5, 65), (1, 7, 130)]
REAL_IDS = ["B%dxH%dxW%d" % s for s in REAL_SHAPES]
ACTS = {"none": lh.ACT_NONE, "tanh": lh.ACT_TANH, "sine": lh.ACT_SINE}


@functools.lru_cache(maxsize=None)
def _real_inputs(B, H, W):
    seed = 7 + (B * 1000 + H) * 1000 + W
    # x and the prior dx are bf16 values, so both dtypes read the same numbers; yout is a saved tanh output, unrelated to dout
    return dict(x=_randn((B, H, W, C), seed).bfloat16().float(), kw=_randn((9, C), seed + 1) / 16, tb=_randn((10,), seed + 2),
                dout=_randn((B, 1, H, W), seed + 3), yout=torch.tanh(_randn((B, 1, H, W), seed + 4)),
                prior=_randn((B, H, W, C), seed + 5).bfloat16().float())


@functools.lru_cache(maxsize=None)
def _real_ref(kind, act, B, H, W):
    i = _real_inputs(B, H, W)
    yout = i["yout"] if act == lh.ACT_TANH else None
    if kind == "fwd":
        return lh.fwd(i["x"], i["kw"], i["tb"], act)
    if kind == "data":
        return lh.bwd_data(i["dout"], yout, i["kw"], act)
    if kind == "data_acc":
        return lh.bwd_data(i["dout"], yout, i["kw"], act, prior=i["prior"])
    return lh.bwd_weight(i["x"], i["dout"], yout, act)


def _check_bound(what, out, ref, S, n, extra=0.0, bf16_out=False):
    n = torch.as_tensor(n, dtype=torch.float64)
    assert n.max().item() <= 16384
    bound = n * lh.U32 * S + extra
    if bf16_out:
        bound = bound + lh.half_ulp_bf16(ref)
    ratio, bad = lh.worst_ratio(out.cpu(), ref, bound)
    print(f"{what}: worst error / bound = {ratio:.4f}")
    assert bad == 0, f"{what}: {bad} elements over their bound, worst error / bound = {ratio:.3f}"


@pytest.mark.parametrize("act", ["none", "tanh", "sine"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", REAL_SHAPES, ids=REAL_IDS)
def test_linear_head_fwd_bounded(B, H, W, dtype, act):
    i = _real_inputs(B, H, W)
    out = _ops().linear_head_fwd(i["x"].to(dtype).cuda(), i["kw"].cuda(), i["tb"].cuda(), ACTS[act])
    ref, S, n = _real_ref("fwd", ACTS[act], B, H, W)
    # |act'| <= 1 for all three, so the bound of the sum carries through; tanhf / sinf add their own 2^-21
    _check_bound(f"fwd {act} {DT_IDS[DTYPES.index(dtype)]} B{B} H{H} W{W}", out, ref, S, n, extra=0.0 if act == "none" else 2.0 ** -21)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("act", ["none", "tanh"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", REAL_SHAPES, ids=REAL_IDS)
def test_linear_head_bwd_data_bounded(B, H, W, dtype, act, accumulate):
    i = _real_inputs(B, H, W)
    dx, buf = _guarded(i["prior"] if accumulate else torch.full((B, H, W, C), float("nan")), dtype)
    yout = i["yout"].cuda()                       # act none: present and ignored
    _ops().linear_head_bwd_data(i["dout"].cuda(), yout, i["kw"].cuda(), dx, ACTS[act], accumulate)
    ref, S, n = _real_ref("data_acc" if accumulate else "data", ACTS[act], B, H, W)
    _check_bound(f"bwd_data {act} {DT_IDS[DTYPES.index(dtype)]} {'acc' if accumulate else 'ovw'} B{B} H{H} W{W}", dx, ref, S, n,
                 bf16_out=dtype == torch.bfloat16)
    assert _guards_intact(buf)


@pytest.mark.parametrize("act", ["none", "tanh"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", REAL_SHAPES, ids=REAL_IDS)
def test_linear_head_bwd_weight_bounded(B, H, W, dtype, act):
    i = _real_inputs(B, H, W)
    R = _ops().linear_head_bwd_weight(i["x"].to(dtype).cuda(), i["dout"].cuda(), i["yout"].cuda(), ACTS[act])
    ref, S, n = _real_ref("weight", ACTS[act], B, H, W)
    mono = 2 if act == "tanh" else 1
    assert bool(((n == 0) | (n >= 3 * mono)).all())      # the condition under which n * 2^-24 * S is a bound
    _check_bound(f"bwd_weight {act} {DT_IDS[DTYPES.index(dtype)]} B{B} H{H} W{W}", R, ref, S, n)


# ---------------------------------------------------------------------------------------------- linear head: refusals
def _raises(match):
    return pytest.raises(RuntimeError, match=match)


def test_linear_head_refusals_return_the_library_error():
    """C = 128, sine in either backward, tanh without the saved output: the wrapper raises the library's error, nothing is launched
    (dx and the result keep their contents), and the next valid call works"""
    ops = _ops()
    B, H, W = 1, 2, 3
    x128 = torch.zeros((B, H, W, 128), device="cuda")
    kw128, tb = torch.zeros((9, 128), device="cuda"), torch.zeros(10, device="cuda")
    dout = torch.ones((B, 1, H, W), device="cuda")
    yout = torch.zeros((B, 1, H, W), device="cuda")
    with _raises("C must be 256"):
        ops.linear_head_fwd(x128, kw128, tb, lh.ACT_NONE)
    dx128, buf128 = _guarded(torch.full((B, H, W, 128), SENTINEL))
    with _raises("C must be 256"):
        ops.linear_head_bwd_data(dout, None, kw128, dx128, lh.ACT_NONE, False)
    with _raises("C must be 256"):
        ops.linear_head_bwd_weight(x128, dout, None, lh.ACT_NONE)
    x, kw = torch.ones((B, H, W, C), device="cuda"), torch.ones((9, C), device="cuda")
    dx, buf = _guarded(torch.full((B, H, W, C), SENTINEL))
    for dtype in DTYPES:
        with _raises("sine backward is not implemented"):
            ops.linear_head_bwd_data(dout, yout, kw, dx, lh.ACT_SINE, False)
        with _raises("sine backward is not implemented"):
            ops.linear_head_bwd_weight(x.to(dtype), dout, yout, lh.ACT_SINE)
        with _raises("tanh needs the forward output"):
            ops.linear_head_bwd_data(dout, None, kw, dx, lh.ACT_TANH, True)
        with _raises("tanh needs the forward output"):
            ops.linear_head_bwd_weight(x.to(dtype), dout, None, lh.ACT_TANH)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((buf128 == SENTINEL).all())
    out = ops.linear_head_fwd(x, kw, tb, lh.ACT_NONE)                  # the library is still usable: corner pixel = 4 taps * 256
    assert out[0, 0, 0, 0].item() == 4 * C and out[0, 0, 0, 1].item() == 6 * C


# ---------------------------------------------------------------------------------------------- small_gemm
def engine_calls(C_, C1, C3, NB=6):
    """(name, M, N, K, sa, sb, sc, accumulate): every call of ops.small_gemm in engine._linear_head_weights, engine._linear_head_algebra and
    classifier_trainer, in their order, as functions of the head's widths (C, C1, C3 = 256, 512, 1024 in production)"""
    return [
        ("u = W4 W3", 1, C1, C3, (0, 1), (C1, 1), (0, 1), False),
        ("Vc = u W2", 1, C1 * 9, C1, (0, 1), (C1 * 9, 1), (0, 1), False),
        ("Kw = Vc^T W1", 9, C_, C1, (1, 9), (C_, 1), (C_, 1), False),
        ("tb = Vc^T b1", 9, 1, C1, (1, 9), (1, 0), (1, 0), False),
        ("tb9 += u.b2", 1, 1, C1, (0, 1), (1, 0), (0, 0), True),
        ("tb9 += W4.b3", 1, 1, C3, (0, 1), (1, 0), (0, 0), True),
        ("gv = W1 G^T", C1, 9, C_, (C_, 1), (1, C_), (9, 1), False),
        ("gv += b1 n", C1, 9, 1, (1, 0), (0, 1), (9, 1), True),
        ("dW1 = Vc G", C1, C_, 9, (9, 1), (C_, 1), (C_, 1), False),
        ("db1 = Vc n", C1, 1, 9, (9, 1), (1, 0), (1, 0), False),
        ("dW2 = u gv", C1, C1 * 9, 1, (1, 0), (0, 1), (C1 * 9, 1), False),
        ("gu = W2 gv", C1, 1, C1 * 9, (C1 * 9, 1), (1, 0), (1, 0), False),
        ("gu += b2 D", C1, 1, 1, (1, 0), (0, 0), (1, 0), True),
        ("db2 = D u", C1, 1, 1, (1, 0), (0, 0), (1, 0), False),
        ("dW4 = gu W3^T", 1, C3, C1, (0, 1), (1, C1), (0, 1), False),
        ("dW4 += D b3", 1, C3, 1, (0, 0), (0, 1), (0, 1), True),
        ("dW3 = W4^T gu", C3, C1, 1, (1, 0), (0, 1), (C1, 1), False),
        ("db3 = D W4^T", C3, 1, 1, (1, 0), (0, 0), (1, 0), False),
        ("cls dW = dlogit^T logits", 1, 1000, NB, (0, 1), (1000, 1), (0, 1), False),
        ("cls dlogits", NB, 1000, 1, (1, 0), (0, 1), (1000, 1), False),
    ]


def _gemm_id(tag, call):
    return f"{tag}-{re.sub('[^A-Za-z0-9]+', '_', call[0])}-M{call[1]}_N{call[2]}_K{call[3]}"


# reduced widths; between them the contractions are K = 1, 9, 63, 64, 65 (both kernels and the switch at 64) and M*N is odd (45, 63, 35)
GEMM_SIZES = {"C8_C12_C20": (8, 12, 20), "C5_C7_C64": (5, 7, 64), "C8_C64_C65": (8, 64, 65), "C8_C65_C63": (8, 65, 63)}
GEMM_CASES = [pytest.param(*call, id=_gemm_id(tag, call)) for tag, sz in GEMM_SIZES.items() for call in engine_calls(*sz)]
# the long contractions at full size: K = 1024, 512 (N = 4608), 4608 and 512 with a transposed B
GEMM_CASES += [pytest.param(*call, id=_gemm_id("full", call)) for k, call in enumerate(engine_calls(256, 512, 1024)) if k in (0, 1, 11, 14)]


def test_small_gemm_cases_cover_both_kernels_and_the_switch():
    ks = {p.values[3] for p in GEMM_CASES}
    assert {1, 9, 63, 64, 65, 512, 4608} <= ks
    assert any((p.values[1] * p.values[2]) % 4 and p.values[3] >= 64 for p in GEMM_CASES)
    assert any((p.values[1] * p.values[2]) % 4 and p.values[3] < 64 for p in GEMM_CASES)


def _extent(d0, d1, s):
    return 1 + (d0 - 1) * s[0] + (d1 - 1) * s[1]


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("name,M,N,K,sa,sb,sc,accumulate", GEMM_CASES)
def test_small_gemm_engine_strides(name, M, N, K, sa, sb, sc, accumulate, kind):
    """operands exactly as long as the strides reach, each between sentinel guards; the result buffer starts from known contents, so an
    element the call must not touch (accumulate=False included) shows"""
    seed = M * 7919 + N * 104729 + K
    mk = (lambda n, m, s: _ints((n,), m, s)) if kind == "int" else (lambda n, m, s: _randn((n,), s))
    A, B, C0 = mk(_extent(M, K, sa), 2, seed), mk(_extent(K, N, sb), 2, seed + 1), mk(_extent(M, N, sc), 8, seed + 2)
    dA, bufA = _guarded(A)
    dB, bufB = _guarded(B)
    dC, bufC = _guarded(C0)
    ret = _ops().small_gemm(dA, dB, dC, M, N, K, sa, sb, sc, accumulate=accumulate)
    assert ret.data_ptr() == dC.data_ptr()
    ref, ic, S, n = lh.small_gemm(A, B, C0, M, N, K, sa, sb, sc, accumulate)
    got = dC.cpu().double()
    assert _guards_intact(bufA) and _guards_intact(bufB) and _guards_intact(bufC)
    assert torch.equal(dA.cpu(), A) and torch.equal(dB.cpu(), B)
    untouched = torch.ones(C0.numel(), dtype=torch.bool)
    untouched[ic.reshape(-1)] = False
    assert torch.equal(got[untouched], C0.double()[untouched])
    if kind == "int":
        assert S.max().item() < 2 ** 24
        assert torch.equal(got, ref)
    else:
        _check_bound(f"small_gemm {name} M{M} N{N} K{K}", got[ic], ref[ic], S, n)


def test_small_gemm_accumulates_onto_a_one_element_view_and_a_full_tensor():
    """tb[9:10] as the engine passes it (a view into the ten tap biases): only element 9 changes, by exactly the dot product"""
    ops = _ops()
    C1 = 12
    u, b2, tb0 = _ints((C1,), 2, 1), _ints((C1,), 2, 2), _ints((10,), 8, 3)
    tb = tb0.cuda()
    ops.small_gemm(u.cuda(), b2.cuda(), tb[9:10], 1, 1, C1, (0, 1), (1, 0), (0, 0), accumulate=True)
    want = tb0.clone()
    want[9] += (u.double() * b2.double()).sum().float()
    assert torch.equal(tb.cpu(), want)
    gv0, b1, n9 = _ints((C1, 9), 8, 4), _ints((C1,), 2, 5), _ints((9,), 2, 6)
    gv = gv0.cuda()
    ops.small_gemm(b1.cuda(), n9.cuda(), gv, C1, 9, 1, (1, 0), (0, 1), (9, 1), accumulate=True)
    assert torch.equal(gv.cpu(), gv0 + b1[:, None] * n9[None, :])


# ---------------------------------------------------------------------------------------------- segsum
REPS = [1, 3, 4, 5, 7, 8, 577]


def _segsum_pattern(pattern, reps):
    """(numel of x, R, rep_stride, seg_stride, C) of the engine's and the classifiers' four uses"""
    if pattern == "pixels":          # [B, HW, C] summed over pixels (binary_classifier, classifier_trainer, engine.py readout)
        Bn, Cn = 3, 10
        return Bn * reps * Cn, Bn, Cn, reps * Cn, Cn
    if pattern == "images":          # [B, Nt, D] summed over images (the position embedding's gradient)
        Nt, D = 5, 6
        return reps * Nt * D, Nt, Nt * D, D, D
    if pattern == "one_row":         # R = 1, seg_stride 0 (bias gradients)
        D = 37
        return reps * D, 1, D, 0, D
    assert pattern == "one_column"   # C = 1 (classifier_trainer's bias)
    return reps, 1, 1, 0, 1


@pytest.mark.parametrize("io", ["f32_f32", "bf16_f32", "bf16_bf16"])
@pytest.mark.parametrize("pattern", ["pixels", "images", "one_row", "one_column"])
def test_segsum_exact(pattern, io):
    din = torch.float32 if io == "f32_f32" else torch.bfloat16
    dout = torch.bfloat16 if io == "bf16_bf16" else torch.float32
    for reps in REPS:
        numel, R, rs, ss, Cn = _segsum_pattern(pattern, reps)
        x = _ints((numel,), 1 if reps > 64 else 3, reps)          # 577 terms: -1..1 keeps a bf16 result below 256
        dx, bufx = _guarded(x, din)
        for accumulate in (False, True):
            prior = _ints((R, Cn), 8, reps + 1)
            ref, S, _ = lh.segsum(x, R, reps, rs, ss, Cn, prior=prior if accumulate else None)
            assert S.max().item() < 2 ** 24 and (dout == torch.float32 or ref.abs().max().item() < 256)
            o, bufo = _guarded(prior if accumulate else torch.full((R, Cn), float("nan")), dout)
            ret = _ops().segsum(dx, R, reps, rs, ss, Cn, out=o, out_f32=dout == torch.float32, accumulate=accumulate)
            assert ret.data_ptr() == o.data_ptr()
            assert torch.equal(o.cpu().double(), ref), (reps, accumulate)
            assert _guards_intact(bufo) and _guards_intact(bufx)
    # without `out` the wrapper allocates [R, C] of the requested type
    o = _ops().segsum(dx, R, reps, rs, ss, Cn, out_f32=dout == torch.float32)
    assert o.shape == (R, Cn) and o.dtype == dout


@pytest.mark.parametrize("io", ["f32_f32", "bf16_f32", "bf16_bf16"])
@pytest.mark.parametrize("pattern", ["pixels", "images", "one_row", "one_column"])
def test_segsum_bounded_at_577(pattern, io):
    din = torch.float32 if io == "f32_f32" else torch.bfloat16
    dout = torch.bfloat16 if io == "bf16_bf16" else torch.float32
    reps = 577
    numel, R, rs, ss, Cn = _segsum_pattern(pattern, reps)
    x = _randn((numel,), 3).to(din)
    for accumulate in (False, True):
        prior = _randn((R, Cn), 4).to(dout)
        ref, S, n = lh.segsum(x, R, reps, rs, ss, Cn, prior=prior if accumulate else None)
        o = prior.cuda() if accumulate else torch.full((R, Cn), float("nan"), dtype=dout, device="cuda")
        _ops().segsum(x.cuda(), R, reps, rs, ss, Cn, out=o, out_f32=dout == torch.float32, accumulate=accumulate)
        _check_bound(f"segsum {pattern} {io} {'acc' if accumulate else 'ovw'}", o, ref, S, n, bf16_out=dout == torch.bfloat16)


# ---------------------------------------------------------------------------------------------- fill_cls
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", [384, 385])
@pytest.mark.parametrize("B", [1, 3])
def test_fill_cls(B, D, dtype):
    """row 0 of every image = cls + pos0 rounded once; the other token rows (batch_stride = 3 rows + 5 elements > D) keep their sentinel"""
    bstride = 3 * D + 5
    cls, pos0 = _randn((D,), 1), _randn((D,), 2)
    tokens, buf = _guarded(torch.full((B * bstride,), SENTINEL), dtype)
    _ops().fill_cls(tokens, cls.cuda(), pos0.cuda(), B, bstride, D)
    want = torch.full((B, bstride), SENTINEL, dtype=dtype)
    want[:, :D] = (cls + pos0).to(dtype)              # f32: the same single IEEE addition; bf16: round-to-nearest-even of that f32 sum
    assert torch.equal(tokens.cpu().view(B, bstride), want)
    assert _guards_intact(buf)


# ---------------------------------------------------------------------------------------------- cast, scale_by_device_scalar
SIZES = [1, 255, 256, 257, 16384 * 256 + 3]          # the last one is past the grid cap of 16384 blocks: the grid-stride loop's second trip


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dout", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("din", DTYPES, ids=DT_IDS)
def test_cast_is_one_f32_multiply_and_one_rounding(din, dout, n):
    """scale 1 and 0.5 (a power of two: the product is exact) and 1/3: to_out(f32(src) * f32(scale)), rounded once"""
    src = _randn((n,), n % 1000).to(din)
    d, bufs = _guarded(src)
    for scale in (1.0, 0.5, 1.0 / 3.0):
        o, bufo = _guarded(torch.full((n,), float("nan")), dout)
        ret = _ops().cast(d, dout, scale=scale, out=o)
        assert ret.data_ptr() == o.data_ptr()
        want = (src.float() * torch.tensor(scale, dtype=torch.float32)).to(dout)
        assert torch.equal(o.cpu(), want), scale
        assert _guards_intact(bufo) and _guards_intact(bufs)
    o = _ops().cast(d, dout)
    assert o.dtype == dout and o.shape == src.shape and torch.equal(o.cpu(), src.to(dout))


@pytest.mark.parametrize("n", SIZES)
def test_scale_by_device_scalar_reads_the_scalar_at_run_time(n):
    """bit-equal to src * scalar in f32; the scalar changes on the device between two calls with no host synchronisation in between"""
    src = _randn((n,), 5 + n % 1000)
    d = src.cuda()
    s1, s2 = torch.tensor([1.0 / 3.0]), torch.tensor([-2.7])
    scalar, new = s1.cuda(), s2.cuda()
    torch.cuda.synchronize()
    a = _ops().scale_by_device_scalar(d, scalar)
    scalar.copy_(new)                                  # device-to-device on the same stream: ordered after the first launch, no sync
    b = _ops().scale_by_device_scalar(d, scalar)
    assert a.dtype == torch.float32 and a.shape == src.shape
    assert torch.equal(a.cpu(), src * s1) and torch.equal(b.cpu(), src * s2)
    assert torch.equal(d.cpu(), src)
