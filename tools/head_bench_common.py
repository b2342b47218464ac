"""What tools/mask_head_bench.py and tools/rpn_head_bench.py share: the windowed median timer and the per-launch times from a
module's own marks."""
import statistics

import torch


def timed(fn, windows, iters, warmup=2, per_call=False, before=None):
    """median over the windows of the mean device time of fn() in ms.  One pair of device events spans a window's `iters` calls;
    per_call=True: every call has its own pair and is waited for.  before(): run ahead of every timed span, outside it"""
    for _ in range(warmup):
        if before:
            before()
        fn()
    out = []
    for _ in range(windows):
        tot = 0.0
        for _ in range(iters if per_call else 1):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(1 if per_call else iters):
                fn()
            b.record()
            b.synchronize()
            tot += a.elapsed_time(b)
        out.append(tot / iters)
    return statistics.median(out)


def module_times(step, windows, fwd_end):
    """step(marks): one forward + backward of the module with _marks=marks, two warm-up runs and `windows` measured ones.  Returns
    (launches_ms: the median time of every launch by the mark after it, forward_ms: fwd_start .. the mark `fwd_end`, backward_ms:
    bwd_start .. the last mark, the mark names in order)"""
    per_launch, fwd_ms, bwd_ms, names = {}, [], [], []
    for w in range(2 + windows):
        marks = []
        step(marks)
        torch.cuda.synchronize()
        if w < 2:
            continue
        names = [n for n, _ in marks]
        for (n0, e0), (n1, e1) in zip(marks[:-1], marks[1:]):
            if n1 not in ("fwd_start", "bwd_start"):
                per_launch.setdefault(n1, []).append(e0.elapsed_time(e1))
        ev = dict(marks)
        fwd_ms.append(ev["fwd_start"].elapsed_time(ev[fwd_end]))
        bwd_ms.append(ev["bwd_start"].elapsed_time(marks[-1][1]))
        print(f"window {w - 2}: forward {fwd_ms[-1]:.3f} ms, backward {bwd_ms[-1]:.3f} ms", flush=True)
    launches_ms = {n: round(statistics.median(v), 4) for n, v in per_launch.items()}
    return launches_ms, statistics.median(fwd_ms), statistics.median(bwd_ms), names
