"""The detector's mask head on the device (unmore_amd.mask_head.MaskRCNNConvUpsampleHead.layers and its backward): one JSON line per
run, appended to profiles/mask_head_bench.jsonl.

    python tools/mask_head_bench.py --rois 2048 --dtype bf16

The input is `--rois` seeded ROI features [R,256,14,14] (the recipe's upper bound is 16 images x 128 foreground proposals) and a
seeded gradient of the logits; every time is the median of `--windows` windows of `--iters` calls, between device events.
  launches_ms:   every launch of layers() and of its backward, by the module's own marks (a weight gradient with its unpacking permute).
  forward_ms / backward_ms: the two halves whole; trunk_tflops: the four convolutions and the deconvolution, forward, and the trunk's
                 backward (twice the forward's operations, less the first layer's data gradient when --no-input-grad).
  tail:          the two tail kernels alone on the deconvolution's output D [R*196, 1024]: their times, the bytes each has to move
                 (logits: D once and the logits; backward: D read and written, the dlogits) and the time those bytes take at 8 TB/s;
                 beside them the same tail composed from the library's older ops: ops.pixel_shuffle + ops.head_out_fwd, and
                 ops.head_out_bwd (ReLU mask on) + the inverse ops.pixel_shuffle.
  torch_ms:      the same head from torch's own conv2d / conv_transpose2d on the GPU in the same type (channels_last), forward and
                 backward, parameters and input requiring gradients alike."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from head_bench_common import module_times, timed  # noqa: E402

C, S = 256, 14
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=2048)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-input-grad", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_head_bench.jsonl"))
    args = ap.parse_args()
    from unmore_amd import mask_head, ops
    import mask_head_common as mc
    assert torch.cuda.is_available(), "mask_head_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    es = 2 if dtype == torch.bfloat16 else 4
    R, M = args.rois, args.rois * S * S

    sd = mc.make_params(C, (C,) * 5, seed=args.seed)
    head = mask_head.MaskRCNNConvUpsampleHead(C, conv_dims=(C,) * 5, compute_dtype=dtype)
    head.load_state_dict(sd, strict=True)
    head = head.to(dev)
    x = mc.make_features(R, C, S, seed=args.seed + 1).to(dev).to(dtype).requires_grad_(not args.no_input_grad)
    dl = mc.make_dlogits(R, S, args.seed + 2).to(dev).to(dtype)

    # ---- the module: every launch, the two halves
    launches_ms, forward_ms, backward_ms, names = module_times(lambda marks: head.layers(x, _marks=marks).backward(dl), args.windows,
                                                               "tail_logits")
    trunk_fwd_flop = R * S * S * (4 * C * 9 * C * 2 + 4 * C * C * 2)
    trunk_fwd_ms = sum(launches_ms[n] for n in names if n.startswith("mask_fcn") and "grad" not in n) + launches_ms["deconv"]
    trunk_bwd_ms = sum(v for n, v in launches_ms.items() if n.endswith("grad"))
    trunk_bwd_flop = 2 * trunk_fwd_flop - (R * S * S * C * 9 * C * 2 if args.no_input_grad else 0)
    for p in head.parameters():
        p.grad = None
    x.grad = None

    # ---- the tail alone, fused and composed
    g = torch.Generator().manual_seed(args.seed + 3)
    D0 = torch.randn(M, 4 * C, generator=g).relu().to(dtype).to(dev)
    wp, bp = sd["predictor.weight"].reshape(-1).to(dev), sd["predictor.bias"].to(dev)
    D = D0.clone()
    dl32 = dl.float()
    tail = {}
    tail["logits_ms"] = timed(lambda: mask_head.tail_logits(D0, wp, bp, R, S), args.windows, args.iters)
    print(f"tail_logits {tail['logits_ms']:.4f} ms", flush=True)
    phases = {}

    def bwd_fused():
        mask_head.tail_bwd(D, dl, wp, R, S, _phase_ms=phases)
    reps = []
    for w in range(2 + args.windows):
        phases.clear()
        D.copy_(D0)
        bwd_fused()
        if w >= 2:
            reps.append(dict(phases))
    tail["bwd_ms"] = statistics.median(r["tail_bwd"] for r in reps)
    tail["bwd_finish_ms"] = statistics.median(r["tail_finish"] for r in reps)
    print(f"tail_bwd {tail['bwd_ms']:.4f} ms + finish {tail['bwd_finish_ms']:.4f} ms", flush=True)
    logits_bytes = M * 4 * C * es + 4 * M * es
    bwd_bytes = 2 * M * 4 * C * es + 4 * M * es
    tail["logits_bytes"], tail["bwd_bytes"] = logits_bytes, bwd_bytes
    tail["logits_ms_at_8TBs"], tail["bwd_ms_at_8TBs"] = logits_bytes / HBM_BYTES_PER_S * 1e3, bwd_bytes / HBM_BYTES_PER_S * 1e3

    wrow = wp.view(1, C).contiguous()
    dw, db = torch.zeros(1, C, device=dev), torch.zeros(1, device=dev)

    def fwd_composed():
        y = ops.pixel_shuffle(D0, R, S, S, 2, C)
        return y, ops.head_out_fwd(y.view(4 * M, C), wrow, bp, R, 2 * S, 2 * S, 0)
    y, yout = fwd_composed()

    def bwd_composed():
        dh = ops.head_out_bwd(y.view(4 * M, C), wrow, dl32, yout, 0, True, dw, db)
        return ops.pixel_shuffle(dh.view(R, 2 * S, 2 * S, C), R, S, S, 2, C, inverse=True)
    tail["composed_logits_ms"] = timed(lambda: fwd_composed(), args.windows, args.iters)
    tail["composed_bwd_ms"] = timed(lambda: bwd_composed(), args.windows, args.iters)
    tail["composed_bwd_inverse_shuffle_only_ms"] = timed(
        lambda: ops.pixel_shuffle(y, R, S, S, 2, C, inverse=True), args.windows, args.iters)
    print(f"composed: logits {tail['composed_logits_ms']:.4f} ms, backward {tail['composed_bwd_ms']:.4f} ms", flush=True)
    # the two forms agree
    D.copy_(D0)
    G, dwp, dbp = mask_head.tail_bwd(D, dl, wp, R, S)
    dw.zero_()
    db.zero_()
    Gc = bwd_composed()
    tail["max_abs_diff_logits"] = float((mask_head.tail_logits(D0, wp, bp, R, S, out_f32=True) - yout).abs().max())
    tail["max_abs_diff_G"] = float((G.float() - Gc.float()).abs().max())
    tail["max_rel_diff_dwp"] = float(((dwp - dw.view(-1)).abs().max() / dw.abs().max()))
    del y, yout, Gc, G, D

    # ---- torch's own convolutions
    torch_ms = None
    if not args.no_torch:
        tw = {k: v.to(dev).to(dtype).requires_grad_(True) for k, v in sd.items()}
        xt = x.detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(not args.no_input_grad)
        out = {}

        def torch_fwd():
            out["logits"] = mc.head_logits(xt, tw, 4)

        def torch_both():
            torch_fwd()
            out["logits"].backward(dl)
        print("torch: warm-up (MIOpen picks its kernels)", flush=True)
        f_ms = timed(torch_fwd, args.windows, args.iters)
        print(f"torch forward {f_ms:.3f} ms", flush=True)
        b_ms = timed(torch_both, args.windows, args.iters)
        torch_ms = {"forward": round(f_ms, 3), "forward_backward": round(b_ms, 3)}
        print(f"torch forward + backward {b_ms:.3f} ms", flush=True)

    line = {"tool": "mask_head_bench", "rois": R, "side": S, "channels": C, "dtype": args.dtype, "f32_mode": ops.get_f32_mode(),
            "windows": args.windows, "iters": args.iters, "input_grad": not args.no_input_grad,
            "forward_ms": round(forward_ms, 3), "backward_ms": round(backward_ms, 3), "launches_ms": launches_ms,
            "trunk_tflops": {"forward": round(trunk_fwd_flop / (trunk_fwd_ms * 1e-3) / 1e12, 1),
                             "backward": round(trunk_bwd_flop / (trunk_bwd_ms * 1e-3) / 1e12, 1)},
            "tail": {k: (round(v, 4) if isinstance(v, float) and v > 1e-3 else v) for k, v in tail.items()},
            "torch_ms": torch_ms, "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
