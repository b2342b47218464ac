"""The RPN head on the device (unmore_amd.rpn_head.StandardRPNHead and its backward): one JSON line per run, appended to
profiles/rpn_head_bench.jsonl.

    python tools/rpn_head_bench.py --images 16 --dtype bf16

The input is p2..p6 of `--images` images of 800 x 1216 (strides 4..64), C = 256, A = 3, seeded; every time is the median of `--windows`
windows between device events.
  launches_ms:   every launch of the head's forward and backward, by the module's own marks.
  forward_ms / backward_ms: the two halves whole; trunk_tflops: the five 3x3 convolutions forward, and their weight and data gradients.
  tail:          the two predictor kernels alone on the stacked hidden map T [M, 256]: their times (the backward with the gradient maps of a
                 real rpn_losses call, and with dense random ones), the bytes each has to move (predict: T once and the 15 output channels;
                 backward: T read and written, the 15 gradient channels) and the time those bytes take at 8 TB/s; beside them, in the same
                 process, the two compositions available without them: torch's own 1x1 conv2d on channels_last maps with autograd (and the
                 ReLU mask as threshold_backward), and the library's gemm_nt / gemm_tn with the predictor weights zero-padded to the
                 narrowest N they accept plus the permutes to and from the NCHW maps.
  nonzero_rows:  the fraction of rows of T whose real gradient is not all zero (what a sparse backward could skip).
  torch_ms:      the whole head from torch's own conv2d (channels_last), forward and forward + backward."""
import argparse
import json
import os
import functools
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import head_bench_common  # noqa: E402

timed = functools.partial(head_bench_common.timed, per_call=True)

C, A = 256, 3
STRIDES = (4, 8, 16, 32, 64)
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_head_bench.jsonl"))
    args = ap.parse_args()
    from unmore_amd import ops, rpn, rpn_head, rpn_loss
    import rpn_head_common as hc
    assert torch.cuda.is_available(), "rpn_head_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    es = 2 if dtype == torch.bfloat16 else 4
    N = args.images
    sizes = [(-(-args.height // s), -(-args.width // s)) for s in STRIDES]
    M = sum(N * h * w for h, w in sizes)
    g = torch.Generator(device=dev).manual_seed(args.seed)

    sd = hc.make_params(C, A, seed=args.seed)
    head = rpn_head.StandardRPNHead(C, A, compute_dtype=dtype)
    head.load_state_dict(sd, strict=True)
    head = head.to(dev)
    feats = [torch.randn(N, C, h, w, generator=g, device=dev).to(dtype).requires_grad_(True) for h, w in sizes]

    # ---- the gradient maps of a real loss, and dense ones
    cells = rpn.cell_anchors([[32], [64], [128], [256], [512]], [0.5, 1.0, 2.0])
    cpu = torch.Generator().manual_seed(args.seed + 1)
    gts = []
    for _ in range(N):
        side = torch.rand(8, generator=cpu) * 300 + 24
        x1, y1 = torch.rand(8, generator=cpu) * (args.width - side), torch.rand(8, generator=cpu) * (args.height - side)
        gts.append(torch.stack([x1, y1, x1 + side, y1 + side * 0.7], dim=1).to(dev))
    image_sizes = [(args.height, args.width)] * N
    with torch.no_grad():
        lg, dl = head(feats)
    lg, dl = [t.requires_grad_(True) for t in lg], [t.requires_grad_(True) for t in dl]
    samples = rpn_loss.label_and_sample_anchors(cells, list(STRIDES), sizes, gts, image_sizes, seed=args.seed)
    losses = rpn_loss.rpn_losses(lg, dl, samples, cells, list(STRIDES), gts)
    (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    real = ([t.grad.contiguous() for t in lg], [t.grad.contiguous() for t in dl])
    rows = torch.cat([hc.stack_rows([a]).ne(0).any(1) | hc.stack_rows([b]).ne(0).any(1) for a, b in zip(*real)])
    nonzero_rows = float(rows.double().mean())
    dense = ([torch.randn(t.shape, generator=g, device=dev).mul_(0.01).to(dtype) for t in lg],
             [torch.randn(t.shape, generator=g, device=dev).mul_(0.01).to(dtype) for t in dl])
    del lg, dl, losses, samples
    print(f"M = {M} rows, {nonzero_rows:.5f} of them with a non-zero real gradient", flush=True)

    # ---- the module: every launch, the two halves
    def step(marks):
        a, b = head(feats, _marks=marks)
        torch.autograd.backward(a + b, real[0] + real[1])
    launches_ms, forward_ms, backward_ms, _ = head_bench_common.module_times(step, args.windows, "predict")
    trunk_flop = M * C * 9 * C * 2
    trunk_fwd_ms = sum(v for n, v in launches_ms.items() if n.startswith("conv_l"))
    trunk_bwd_ms = sum(v for n, v in launches_ms.items() if n.startswith("conv_wgrad") or n.startswith("conv_dgrad"))
    for p in head.parameters():
        p.grad = None
    for f in feats:
        f.grad = None

    # ---- the predictors alone, fused and composed
    T0 = torch.randn(M, C, generator=g, device=dev).relu_().to(dtype)
    T = T0.clone()
    wo, bo, wd, bd = (sd[k].to(dev) for k in ("objectness_logits.weight", "objectness_logits.bias", "anchor_deltas.weight", "anchor_deltas.bias"))
    tail = {}
    tail["predict_ms"] = timed(lambda: rpn_head.predict(T0, sizes, N, wo, bo, wd, bd), args.windows, args.iters)
    print(f"predict {tail['predict_ms']:.4f} ms", flush=True)
    for label, maps in (("real", real), ("dense", dense)):
        reps = []
        for w in range(2 + args.windows):
            phases = {}
            T.copy_(T0)
            rpn_head.predict_bwd(T, sizes, N, maps[0], maps[1], wo, wd, _phase_ms=phases)
            if w >= 2:
                reps.append(phases)
        tail[f"bwd_{label}_ms"] = statistics.median(r["predict_bwd"] for r in reps)
        tail[f"bwd_{label}_finish_ms"] = statistics.median(r["predict_finish"] for r in reps)
        print(f"predict_bwd ({label} gradients) {tail[f'bwd_{label}_ms']:.4f} ms + finish {tail[f'bwd_{label}_finish_ms']:.4f} ms", flush=True)
    tail["predict_bytes"] = M * C * es + M * 5 * A * es
    tail["bwd_bytes"] = 2 * M * C * es + M * 5 * A * es
    tail["predict_ms_at_8TBs"], tail["bwd_ms_at_8TBs"] = tail["predict_bytes"] / HBM_BYTES_PER_S * 1e3, tail["bwd_bytes"] / HBM_BYTES_PER_S * 1e3

    # the library's GEMMs on zero-padded weights, with the permutes to and from NCHW
    first, at = [], 0
    for h, w in sizes:
        first.append(at)
        at += N * h * w
    wcat = torch.cat([wo.reshape(A, C), wd.reshape(4 * A, C)])
    bcat = torch.cat([bo, bd])
    npad = None
    for cand in (16, 32, 64, 128, 256):
        wp = torch.zeros(cand, C, device=dev)
        wp[:5 * A] = wcat
        try:
            ops.gemm_nt(T0[:4096], wp.to(dtype), torch.zeros(cand, device=dev))
            ops.gemm_tn(T0[:4096, :cand].contiguous(), T0[:4096])
            npad = cand
            break
        except (RuntimeError, AssertionError):
            continue
    tail["composed_gemm_npad"] = npad
    if npad is not None:
        wpad = torch.zeros(npad, C, device=dev)
        wpad[:5 * A] = wcat
        bpad = torch.zeros(npad, device=dev)
        bpad[:5 * A] = bcat
        wpad_c, wpad_t = wpad.to(dtype), wpad.t().contiguous().to(dtype)
        out_l = [torch.empty(N, A, h, w, dtype=dtype, device=dev) for h, w in sizes]
        out_d = [torch.empty(N, 4 * A, h, w, dtype=dtype, device=dev) for h, w in sizes]
        gp = torch.zeros(M, npad, dtype=dtype, device=dev)
        zpad = [torch.zeros(N, npad - 5 * A, h, w, dtype=dtype, device=dev) for h, w in sizes]

        def gemm_fwd():
            y = ops.gemm_nt(T0, wpad_c, bpad)
            for k, (h, w) in enumerate(sizes):
                ops.permute4(y, out_l[k], (N, A, h, w), (h * w * npad, 1, w * npad, npad), src_offset=first[k] * npad)
                ops.permute4(y, out_d[k], (N, 4 * A, h, w), (h * w * npad, 1, w * npad, npad), src_offset=first[k] * npad + A)

        def gemm_bwd(maps):
            for k, (h, w) in enumerate(sizes):                   # [N, 5A -> npad, H, W] by torch.cat, then NCHW -> the rows of the level
                both = torch.cat([maps[0][k], maps[1][k], zpad[k]], dim=1)
                ops.permute4(both, gp[first[k]:first[k] + N * h * w], (N, h, w, npad), (npad * h * w, w, 1, h * w))
            G = ops.gemm_nt(gp, wpad_t, aux=T0, mask_relu=True)
            db = torch.empty(npad, device=dev)
            return G, ops.gemm_tn(gp, T0, dbias=db), db
        try:
            tail["composed_gemm_predict_ms"] = timed(gemm_fwd, args.windows, args.iters)
            tail["composed_gemm_bwd_ms"] = timed(lambda: gemm_bwd(real), args.windows, args.iters)
            fused = rpn_head.predict(T0, sizes, N, wo, bo, wd, bd)
            tail["composed_gemm_max_abs_diff"] = max(float((a.float() - b.float()).abs().max()) for a, b in zip(fused[0] + fused[1], out_l + out_d))
            print(f"library GEMMs, N padded to {npad}: predict {tail['composed_gemm_predict_ms']:.4f} ms, backward "
                  f"{tail['composed_gemm_bwd_ms']:.4f} ms", flush=True)
        except (RuntimeError, AssertionError) as e:      # a strided destination the permute refuses: say so instead of a number
            tail["composed_gemm_error"] = str(e)[:200]
            print(f"library GEMM composition failed: {e}", flush=True)
        del gp, out_l, out_d, zpad

    # torch's own 1x1 convolutions on the hidden maps
    if not args.no_torch:
        import torch.nn.functional as F
        hid = [T0[first[k]:first[k] + N * h * w].view(N, h, w, C).permute(0, 3, 1, 2).requires_grad_(True) for k, (h, w) in enumerate(sizes)]
        tw = [t.to(dtype).requires_grad_(True) for t in (wo, bo, wd, bd)]
        keep = {}

        def torch_fwd():
            keep["out"] = [F.conv2d(x, tw[0], tw[1]) for x in hid] + [F.conv2d(x, tw[2], tw[3]) for x in hid]

        def torch_bwd():
            grads = torch.autograd.grad(keep["out"], hid + tw, [m.to(dtype) for m in real[0] + real[1]], retain_graph=True)
            return [torch.ops.aten.threshold_backward(gh, x, 0) for gh, x in zip(grads, hid)]
        tail["torch_predict_ms"] = timed(torch_fwd, args.windows, args.iters)
        tail["torch_bwd_ms"] = timed(torch_bwd, args.windows, args.iters)
        print(f"torch 1x1 conv2d: predict {tail['torch_predict_ms']:.4f} ms, backward {tail['torch_bwd_ms']:.4f} ms", flush=True)
        del hid, keep
    del T, T0

    # ---- the whole head from torch's own convolutions
    torch_ms = None
    if not args.no_torch:
        tw = {k: v.to(dev).to(dtype).requires_grad_(True) for k, v in sd.items()}
        xt = [f.detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True) for f in feats]
        out = {}

        def torch_fwd():
            out["maps"] = hc.head_chain(xt, tw)

        def torch_both():
            torch_fwd()
            torch.autograd.backward(out["maps"][0] + out["maps"][1], real[0] + real[1])
        print("torch: warm-up (MIOpen picks its kernels)", flush=True)
        f_ms = timed(torch_fwd, args.windows, args.iters)
        b_ms = timed(torch_both, args.windows, args.iters)
        torch_ms = {"forward": round(f_ms, 3), "forward_backward": round(b_ms, 3)}
        print(f"torch forward {f_ms:.3f} ms, forward + backward {b_ms:.3f} ms", flush=True)

    line = {"tool": "rpn_head_bench", "images": N, "height": args.height, "width": args.width, "channels": C, "anchors": A, "rows": M,
            "dtype": args.dtype, "f32_mode": ops.get_f32_mode(), "windows": args.windows, "iters": args.iters,
            "forward_ms": round(forward_ms, 3), "backward_ms": round(backward_ms, 3), "launches_ms": launches_ms,
            "trunk_tflops": {"forward": round(trunk_flop / (trunk_fwd_ms * 1e-3) / 1e12, 1),
                             "backward": round(2 * trunk_flop / (trunk_bwd_ms * 1e-3) / 1e12, 1)},
            "tail": {k: (round(v, 4) if isinstance(v, float) and v > 1e-3 else v) for k, v in tail.items()},
            "nonzero_rows": nonzero_rows, "torch_ms": torch_ms, "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
