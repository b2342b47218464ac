"""Headline benchmark: images/sec of one ObjectnessNet training step (forward + 4-term
loss + backward + gradient all-reduce + Adam) on synthetic 384x384 batches.

    python bench.py --gpus N --steps K --warmup W                  (N > 1: this process only starts N rank processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One process per GPU (RCCL over xGMI for N > 1), weak scaling (fixed per-GPU batch).
Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the --steps steps and prints the headline (`value`,
`ms_per_step`, ...).  Everything else this file measures runs only with `--full`:
  roofline     -- the dominant kernel (the implicit-GEMM 3x3 conv 512->512 of the heads),
                  timed live with HIP events on its launch stream;
  cpu_baseline -- the CPU oracle on the host cores (rank 0, N == 1 only);
  alt_*        -- the non-headline forms of the same workload (other sdf-head forms, precisions);
  the host's enqueue time into a drained queue, and (N > 1) the traced gradient exchange of one more step.
`--dump-outputs DIR` writes what the timed path returned in its last timed step as DIR/<name>.npy (rank 0).

Workloads (BASELINE.json configs): cfg2 (default; configs[1], the one the metric is quoted on; configs[2] is the same at
N = 8), cfg1 (configs[0]: ViT-S/16 224x224 batch 2 forward only), cfg4 (configs[3]: ViT-L/14 518x518 batch 16 train step),
ref (the reference's own training recipe: dpt_large, 128x128, batch 20),
cfg5 (configs[4]: the object_reasoning.py inference sweep -- per 640x480 image the 1,225 anchors of :109-137 as 128x128 crops in
batches of 50 through crop+resize, the net, centre peak picking and boundary deltas; one step = one image), tiny (plumbing).
`--rehearse` runs the multi-process plumbing alone on CPU tensors (rendezvous, barrier, bucketed all-reduce of a gradient
buffer of the workload's size, max-over-ranks timing) -- no model, no `value`; it exists so that the N > 1 launch path of this
file is covered by a world_size-2 gloo test in a container without a GPU.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {
    "cfg1": dict(kind="forward", backbone="dpt_small", H=224, W=224, batch=2, name="ObjectnessNet ViT-S/16 224x224 batch=2 forward-only"),
    # BASELINE.json configs[1]: the configuration the metric is quoted on
    "cfg2": dict(kind="train", backbone="dpt_base", H=384, W=384, batch=64, name="ObjectnessNet ViT-B/16 384x384 bf16 batch=64 train"),
    "cfg4": dict(kind="train", backbone="dpt_large14", H=518, W=518, batch=16, name="ObjectnessNet ViT-L/14 518x518 bf16 batch=16 train"),
    "cfg5": dict(kind="sweep", backbone="dpt_base", H=128, W=128, batch=50, image=(480, 640), proposals=1225,
                 name="object_reasoning sweep: ViT-B/16 maps on 640x480 images, 1225 proposals/image as 128x128 crops in batches of 50"),
    # the reference's own recipe (README.md:150-154, train_objectness_net.py:783-788,815-817): dpt_large, 128x128, batch 20
    "ref": dict(kind="train", backbone="dpt_large", H=128, W=128, batch=20, name="ObjectnessNet ViT-L/16 (dpt_large) 128x128 bf16 batch=20 train (the reference's recipe)"),
    "tiny": dict(kind="train", backbone="dpt_tiny", H=64, W=64, batch=2, name="miniature plumbing config"),
}
# what the reference itself has for each backbone name: said next to every number of an extension config
REFERENCE_STATUS = {
    "dpt_large": "the reference's own backbone (objectness_net.py:62-73)",
    "dpt_base": "the reference's DPT wiring 'vitb16_384' (models/dpt/models.py:45, blocks.py:45-54) under a backbone_type name this build adds; "
                "ObjectnessNet's own switch (objectness_net.py:51-107) does not offer it",
    "dpt_small": "EXTENSION: no ViT-S/16 in the reference; DPT-small convention (D 384, hooks [2,5,8,11], features [48,96,192,384]); semantics are this build's",
    "dpt_large14": "EXTENSION: no patch-14 backbone in the reference (patch size 16 is hard-coded, models/dpt/vit.py:262,339; an odd token grid breaks its skip "
                   "additions, blocks.py:372); resizing to the skip's size and the 37x37 position grid are this build's semantics -- no reference result exists "
                   "for this configuration",
    "dpt_tiny": "miniature of the reference's wiring for plumbing tests",
}
SWEEP_CHECK = (600, 620)   # cfg5: the proposals the CPU oracle is TIMED on (20 of 1225: a bounded sample)
# cfg5: the proposals whose peak indices the CPU oracle re-derives (untimed): every sixth anchor of the 32-pixel grid (proposals
# 0..899) and every anchor of the 64 / 128 / 256 / 512-pixel grids plus the whole image (900..1224, object_reasoning.py:109-137)
# -- each anchor scale and shape is covered
SWEEP_CHECK_IDX = sorted(set(range(0, 900, 6)) | set(range(900, 1140, 3)) | set(range(1140, 1225)))
PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
DUMP_BYTES = 64 * 10 ** 6  # --dump-outputs: at most this many bytes of .npy files in all, headers included
NPY_HEADER_BYTES = 4096    # per file: an upper bound of an .npy header (128 bytes for the shapes written here)


def forward_gflop_per_image(cfg, H, W):
    """SURVEY.md section 8d formula (2*MAC, forward)."""
    p, D, L_ = cfg["patch"], cfg["D"], max(cfg["hooks"]) + 1
    Fs = cfg["features"]
    gh, gw = H // p, W // p
    g = gh * gw
    N = g + 1
    P = [16 * g, 4 * g, g, ((gh - 1) // 2 + 1) * ((gw - 1) // 2 + 1)]
    out = H * W
    fl = 2 * g * 3 * p * p * D + L_ * (24 * N * D * D + 4 * N * N * D) + 16 * g * D * D
    fl += 2 * g * D * sum(Fs) + 2 * (16 * g * Fs[0] ** 2 + 4 * g * Fs[1] ** 2 + 9 * P[3] * Fs[3] ** 2)
    fl += 2 * 9 * 256 * sum(P[i] * Fs[i] for i in range(4))
    c3, c1 = 9 * 256 * 256, 256 * 256
    fl += 2 * ((2 * c3 * P[3] + c1 * 4 * P[3]) + (4 * c3 * P[2] + c1 * P[1]) + (4 * c3 * P[1] + c1 * P[0]) + (4 * c3 * P[0] + c1 * 4 * P[0]))
    fl += 2 * out * (2 * (256 * 512 + 9 * 512 * 512 + 512 * 1024) + 1024 * 3)
    return fl / 1e9


def anchors(height, width):
    """the proposal grid of object_reasoning.py:109-137: 5 grid sizes x 3 anchor shapes around every grid point, clipped to the
    image, plus the whole image (1,225 boxes for 640x480)."""
    import numpy as np
    out = []
    for gs in (32, 64, 128, 256, 512):
        xc, yc = np.meshgrid(np.arange(0, width, gs, dtype=int), np.arange(0, height, gs, dtype=int))
        c = np.stack([xc.flatten(), yc.flatten(), xc.flatten(), yc.flatten()]).transpose().reshape(-1, 1, 4)
        base = np.array([[-gs, -gs, gs, gs], [-gs / 2, -gs, gs / 2, gs], [-gs, -gs / 2, gs, gs / 2]]).reshape(1, -1, 4)
        out.append((c + base).reshape(-1, 4))
    out = np.concatenate(out, 0).astype(np.float64)
    out[:, 0][out[:, 0] < 0] = 0
    out[:, 1][out[:, 1] < 0] = 0
    out[:, 2][out[:, 2] >= width] = width
    out[:, 3][out[:, 3] >= height] = height
    return np.concatenate((out, [[0, 0, width, height]]), 0)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: one out_dir/<name>.npy per array, float64 where the path returns float64 or integers (exact), float32
    otherwise.  An array whose file would exceed its equal share of DUMP_BYTES is written as a fixed, seeded sample of its
    flattened elements: the same positions in every run with the same arguments, so two builds compare element for element."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BYTES // max(len(arrays), 1) - NPY_HEADER_BYTES     # data bytes per file
    for name, t in arrays.items():
        wide = t.dtype in (torch.float64, torch.int64, torch.int32)
        t = t.detach()
        item = 8 if wide else 4
        if t.numel() * item > share:
            rng = np.random.default_rng(1234)
            pos = np.unique(rng.integers(0, t.numel(), share // item))
            t = t.reshape(-1)[torch.from_numpy(pos).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.to("cpu", torch.float64 if wide else torch.float32).numpy())


# ----------------------------------------------------------------------------------------------- CPU baseline
def _host():
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    # threads = this process's CPU share, capped at 16 (a 1-GPU box exposes all host cores but grants 16; oversubscribing
    # 256 threads made one step ~50x slower)
    cores = max(1, min(cores, 16))
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return cores, model


def cpu_baseline(wl, hip_peaks=None):
    """the CPU restatement (oracle: fp32 PyTorch ops, autograd, Adam) of the same workload on the host
    cores, torch threads = the process's CPU share; 2 warm-ups, median of >= 5 timed iterations (3 when one iteration takes
    longer than 12 s).  Train workloads: the full step (fwd + loss + bwd + Adam) on ONE image of the workload's own
    resolution (a batch of 64 does not fit the time budget; every image is independent, so images/sec = 1 / step time).
    cfg1: the whole workload (forward, batch 2).  cfg5: crop+resize, forward, peak picking and box deltas on 10 of an
    image's 1,225 proposals; images/sec = (10 / time) / 1225."""
    import numpy as np
    import torch
    from oracle import objectness_oracle as orc
    from unmore_amd import synth
    from unmore_amd.hashrng import hash_init
    cores, model = _host()
    torch.set_num_threads(cores)
    cfg = orc.CONFIGS[wl["backbone"]]
    spec = orc.state_dict_spec(cfg)
    kind = wl["kind"]
    H, W = wl["H"], wl["W"]
    if kind == "train":
        sd = {k: torch.from_numpy(hash_init(k, s, "bench")).requires_grad_(True) for k, s in spec.items()}
        img, cf, sdf, sal = (torch.from_numpy(a) for a in synth.make_batch(1, H, W, seed=123))
        m = {k: torch.zeros_like(v) for k, v in sd.items()}
        v = {k: torch.zeros_like(v_) for k, v_ in sd.items()}
        per_iter, what = 1.0, f"one train step (fwd+loss+bwd+Adam) on 1 image of {H}x{W}"

        def one(step):
            for t in sd.values():
                t.grad = None
            loss, _ = orc.loss_terms(orc.forward(sd, img, cfg), cf, sdf, sal)
            loss.backward()
            with torch.no_grad():
                for k, t in sd.items():
                    if t.grad is not None:
                        orc.adam_update(t, t.grad, m[k], v[k], step)
    elif kind == "forward":
        sd = {k: torch.from_numpy(hash_init(k, s, "bench")) for k, s in spec.items()}
        img = torch.from_numpy(synth.make_batch(wl["batch"], H, W, seed=123)[0])
        per_iter, what = float(wl["batch"]), f"forward of the whole workload ({wl['batch']} images of {H}x{W})"

        def one(step):
            with torch.no_grad():
                orc.forward(sd, img, cfg)
    else:  # sweep: the same net (hash weights + the peak fixtures' documented edits) and the same image as the GPU leg
        sd = {k: torch.from_numpy(v) for k, v in synth.peak_edited_state_dict(spec, "base").items()}
        Hi, Wi = wl["image"]
        image = torch.from_numpy(synth.blob_images(1, Hi, Wi, seed=0)[0])
        lo, hi = SWEEP_CHECK
        props = torch.from_numpy(anchors(Hi, Wi))[lo:hi]
        per_iter, what = (hi - lo) / wl["proposals"], f"crop+resize, forward, peak picking, box deltas on {hi - lo} of one image's 1225 proposals"
        kept = {}

        def one(step):
            with torch.no_grad():
                crops = orc.crop_resize(image, props, 128)
                out = orc.forward(sd, crops, cfg)
                orc.peak_pick(out["sdf_maps"][:, 0], out["center_fields"])
                orc.update_bbox_with_boundary_fields(out["sdf_maps"][:, 0])
                kept["out"] = out

    print(f"[bench] cpu_baseline: timing the CPU oracle ({what}) on {cores} threads ...", file=sys.stderr, flush=True)
    times = []
    for i in range(2):
        t0 = time.perf_counter()
        one(1 + i)
        times.append(time.perf_counter() - t0)
        print(f"[bench] cpu_baseline: warm-up {i + 1}/2 {times[-1]:.1f} s", file=sys.stderr, flush=True)
    n = 5 if times[-1] <= 12.0 else 3
    timed = []
    for i in range(n):
        t0 = time.perf_counter()
        one(3 + i)
        timed.append(time.perf_counter() - t0)
        print(f"[bench] cpu_baseline: iteration {i + 1}/{n} {timed[-1]:.1f} s", file=sys.stderr, flush=True)
    med = float(np.median(timed))
    extra = {}
    if kind == "sweep" and hip_peaks is not None:
        # configs[4]: "peak-picking bit-exact vs CPU" -- the flat argmax of every checked proposal, HIP fp32 sweep vs this CPU
        # oracle on the same crops (untimed pass over SWEEP_CHECK_IDX: every anchor scale); `certified` = proposals whose CPU argmax
        # is provably stable against any field perturbation below 2e-4 (oracle.peak_certificate): a mismatch there would be a real
        # error, elsewhere it is a near-tie
        h_amax, h_arg = hip_peaks
        all_props = torch.from_numpy(anchors(Hi, Wi))
        idx = SWEEP_CHECK_IDX
        n_peak_cpu = n_cert = n_mism = n_mism_cert = 0
        worst_amax = 0.0
        print(f"[bench] cpu_baseline: re-deriving the peaks of {len(idx)} proposals on the CPU oracle (untimed) ...", file=sys.stderr, flush=True)
        for i in range(0, len(idx), 50):
            sel = idx[i:i + 50]
            with torch.no_grad():
                crops = orc.crop_resize(image, all_props[sel], 128)
                out = orc.forward(sd, crops, cfg)
            amax, arg, cert = orc.peak_certificate(out["sdf_maps"][:, 0].contiguous(), out["center_fields"].contiguous(), 2e-4, certify_empty=True)
            for j, k in enumerate(sel):
                mism = int(arg[j]) != int(h_arg[k])
                n_peak_cpu += int(float(amax[j]) > 0)
                n_cert += int(bool(cert[j]))
                n_mism += int(mism)
                n_mism_cert += int(mism and bool(cert[j]))
                worst_amax = max(worst_amax, abs(float(amax[j]) - float(h_amax[k])))
        extra["peak_check"] = {
            "proposals_checked": len(idx), "proposal_set": "every 6th anchor of the 32-px grid, every 3rd of the 64-px grid, every anchor of the 128 / 256 / 512-px grids and the whole image",
            "maps_with_peak_cpu": n_peak_cpu, "maps_with_peak_hip": int((h_amax[idx] > 0).sum()),
            "peak_index_mismatches": n_mism, "certified": n_cert, "mismatches_among_certified": n_mism_cert,
            "max_abs_amax_difference": worst_amax,
            "note": "flat argmax of the eroded anti-centre score map per proposal, the headline HIP fp32 sweep vs the CPU oracle (torch fp32) on the same crops; "
                    "certified = the oracle's argmax is provably stable under any field perturbation < 2e-4 (maps without a positive score included)"}
    return {**extra, "value": per_iter / med, "unit": "images/sec", "cores": cores, "cpu_model": model, "kind": "port",
            "sample": f"median of {n} timed iterations after 2 warm-ups, each = {what}; fp32, torch CPU, {cores} threads; "
                      f"median {med:.2f} s/iteration"}


def measured_traffic(a, M_head):
    """HBM-side bytes per launch of the dominant kernel: PMC counters cannot be read from inside the process, so this is the
    figure of the committed rocprofv3 passes (tools/profile_round.sh: separate --pmc FETCH_SIZE / WRITE_SIZE runs of this
    same command, FETCH doubled for gfx950; profiles/rNN_pmc_traffic[_<workload>].json).  null when no profile matches the run
    (another batch size, or a workload / precision that was never profiled)."""
    if a.batch is not None or a.workload not in ("cfg2", "cfg4", "cfg5"):
        return {"traffic": None}
    if a.dtype != ("fp32" if a.workload == "cfg5" else "bf16"):
        return {"traffic": None}
    import glob
    suffix = "" if a.workload == "cfg2" else "_" + a.workload
    # the head conv runs as <conv, epilogue class 3> (bf16: forward, sdf data gradient; <1, 3, 2>: the ReLU-masked data gradient)
    # or <conv, 5> (fp32 parity mode: bf16-plane operands)
    prefix = "gemm_nt256p_kernel<1, 5" if a.dtype == "fp32" else "gemm_nt256p_kernel<1, 3, 0"
    # algorithmic bytes: one read of the input map + one write of the output map, 512 channels each; bf16 = 2 B per value, planes = 6 B
    per_value = 6.0 if a.dtype == "fp32" else 2.0
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic{suffix}.json")), reverse=True):
        if a.workload == "cfg5" and getattr(a, "sweep_precision", "full") == "certified" and os.path.basename(f) < "r06":
            continue      # (rounds 2-5 profiled the six-term sweep: another kernel mix)
        try:
            for k in json.load(open(f))["kernels"]:
                if k["kernel"].startswith(prefix) and k.get("class") == "large" and "hbm_bytes_per_launch" in k:
                    return {"traffic": k["hbm_bytes_per_launch"], "traffic_unit": "bytes/launch (FETCH_SIZE x2 + WRITE_SIZE)",
                            "traffic_source": os.path.relpath(f, ROOT), "algorithmic_bytes_per_launch": 2.0 * M_head * 512 * per_value}
        except (OSError, ValueError, KeyError):
            continue
    return {"traffic": None}


# ----------------------------------------------------------------------------------------------- rank launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tail(path, nbytes=4000):
    try:
        with open(path, "rb") as f:
            f.seek(0, 2)
            size = f.tell()
            f.seek(max(0, size - nbytes))
            return f.read().decode(errors="replace")
    except OSError:
        return ""


def spawn_ranks(n, timeout_s):
    """`python bench.py --gpus N` called plainly: this parent has not touched the GPU (no torch import); it starts N fresh rank
    processes of this same file with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, passes rank 0's JSON line through and
    exits with the ranks' status.  No exec of anything from a GPU-initialised process.

    The parent never blocks on one child: it polls all of them.  The first rank that exits non-zero (RCCL init failure, OOM,
    an assert) ends the run within seconds -- the ranks this parent started are terminated (they would otherwise sit in a
    collective / the rendezvous until someone kills them), the failing rank's stderr tail is printed and the parent exits with
    that rank's status.  An overall deadline counted from the launch does the same for a hang (exit status 124).  Rank 0's
    stderr is passed through live; every other rank's stderr is kept in a file whose path is printed on failure."""
    import tempfile
    import threading
    env0 = dict(os.environ)
    env0.setdefault("MASTER_ADDR", "127.0.0.1")
    env0["MASTER_PORT"] = env0.get("MASTER_PORT") or str(_free_port())
    env0["WORLD_SIZE"] = str(n)
    env0.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env0.setdefault("NCCL_DEBUG", "WARN")   # RCCL's own warnings land in the ranks' stderr: rank 0 live, the others in the failure tail
    env0.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    logdir = tempfile.mkdtemp(prefix="umr_bench_ranks_")
    t_start = time.time()
    procs, errfiles = [], []
    for r in range(n):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
        ef = open(os.path.join(logdir, f"rank{r}.stderr"), "wb") if r else None
        errfiles.append(ef)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=(subprocess.PIPE if r == 0 else subprocess.DEVNULL), stderr=ef))
    out0 = []
    reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)   # never blocks the poll loop
    reader.start()

    def stop_all():
        for p in procs:
            if p.poll() is None:
                p.terminate()   # exactly the children this parent started
        t_kill = time.time() + 5.0
        for p in procs:
            try:
                p.wait(timeout=max(0.1, t_kill - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()

    rc, why = 0, None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            r, c = bad[0]
            rc, why = (c if c > 0 else 128 - c), f"rank {r} exited with status {c}"
            break
        if all(c == 0 for c in codes):
            break
        if time.time() - t_start > timeout_s:
            running = [r for r, c in enumerate(codes) if c is None]
            rc, why = 124, f"deadline of {timeout_s:.0f} s passed with ranks {running} still running"
            break
        time.sleep(0.1)
    if why is not None:
        stop_all()
        sys.stderr.write(f"[bench] FAILED: {why}; the other ranks were terminated ({time.time() - t_start:.1f} s after launch)\n")
        for r in range(1, n):
            tail = _tail(os.path.join(logdir, f"rank{r}.stderr"))
            if tail.strip():
                sys.stderr.write(f"[bench] ---- rank {r} stderr (tail; full text: {logdir}/rank{r}.stderr)\n{tail}\n")
    reader.join(timeout=5.0)
    for ef in errfiles:
        if ef is not None:
            ef.close()
    # exactly what rank 0 reported goes to stdout: its JSON line; anything a library printed beside it goes to stderr.  After a
    # failure nothing goes to stdout: a line from a run whose ranks did not all finish is not a result.
    for line in (out0[0].decode(errors="replace") if out0 else "").splitlines():
        (sys.stdout if (line.startswith("{") and why is None) else sys.stderr).write(line + "\n")
    sys.stdout.flush()
    sys.stderr.flush()
    return rc


# ----------------------------------------------------------------------------------------------- per-rank body
def run_rank(a):
    import numpy as np
    import torch
    import torch.distributed as dist
    from argparse import Namespace

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    if a.fail_rank is not None and rank == a.fail_rank:
        # launcher test hook: this rank dies before the rendezvous, the others are left waiting in it
        print(f"[bench] rank {rank}: --fail-rank requested, exiting with status 3", file=sys.stderr, flush=True)
        sys.exit(3)
    wl = WORKLOADS[a.workload]
    if a.rehearse:
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench.py needs the MI355X (no CPU fallback)"
        ndev = torch.cuda.device_count()
        assert a.backend == "gloo" or world <= ndev, f"{world} ranks but {ndev} GPUs (RCCL needs one device per rank)"
        torch.cuda.set_device(local % ndev)   # gloo rehearsal on a 1-GPU box: ranks share the device
        dev = torch.device("cuda", local % ndev)
    coll = {"backend": "none", "world": world}
    # UMR_DP_FORCE=1: the data-parallel path in a process group of ONE rank (a builder's box has one GPU and RCCL refuses two ranks on
    # a device): every bucket goes through ProcessGroupNCCL (parallel.BucketedAllReduce(force=...)), the line says so in `collective`
    dist_on = world > 1 or os.environ.get("UMR_DP_FORCE", "0") == "1"
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
            try:
                ver = ".".join(map(str, torch.cuda.nccl.version()))
            except Exception:   # version query is informational only
                ver = "unknown"
            coll = {"backend": "nccl (RCCL)", "world": dist.get_world_size(), "rccl_version": ver}
        else:
            dist.init_process_group("gloo")
            coll = {"backend": "gloo", "world": dist.get_world_size()}

    if dist_on:
        coll["gradient_wire"] = a.dp_wire
        if world == 1:
            coll["forced_single_rank"] = True

    def barrier():
        if dist_on:
            if a.backend == "nccl" and dev.type == "cuda":
                dist.barrier(device_ids=[dev.index])
            else:
                dist.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def max_over_ranks(x):
        if dist_on:
            t = torch.tensor([x], dtype=torch.float64, device=dev if a.backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return x

    def gather_over_ranks(x):
        """every rank's own figure, in rank order (for the per-rank rates in the line)"""
        if dist_on:
            t = torch.zeros(world, dtype=torch.float64, device=dev if a.backend == "nccl" else "cpu")
            t[rank] = x
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return [float(v) for v in t.tolist()]
        return [x]

    if a.rehearse:
        return rehearse(a, wl, world, rank, coll, barrier, max_over_ranks, gather_over_ranks)

    from unmore_amd import ops, reasoning, synth
    from unmore_amd.engine import CONFIGS
    from unmore_amd.objectness_net import ObjectnessNet
    from unmore_amd.trainer import TrainStep

    B = a.batch or wl["batch"]
    H, W = wl["H"], wl["W"]
    cfg = CONFIGS[wl["backbone"]]
    if a.cu_budget:
        ops.set_cu_budget(a.cu_budget)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    kind = wl["kind"]

    torch.manual_seed(0)  # identical random-init weights on every rank
    net = ObjectnessNet(dev, H, wl["backbone"], Namespace(use_bg_sdf=True, sdf_activation="tanh")).to(dev)
    net.set_compute_dtype(dt)
    M_head = B * H * W

    # dominant kernel: 3x3 conv 512->512 over all pixels of the batch (heads; train: 2 forward launches + the centre head's
    # data-gradient launch per step -- the boundary-distance head's backward is algebraic; the weight gradient is the TN kernel)
    def is_head_conv(d):
        return d.conv == 1 and d.Cin == 512 and d.N == 512 and d.M == M_head

    if kind == "train":
        net.train()
        step = TrainStep(net, lr=1e-4, center_field_loss_type="l2", sdf_loss_type="l1", use_sdf_gradient_loss=True,
                         use_sdf_binary_mask_loss=True, lr_milestones=(10000, 20000), lr_gamma=0.1,
                         grad_wire_dtype=(torch.bfloat16 if a.dp_wire == "bf16" else None))
        img, cf, sdf, sal = (torch.from_numpy(x).to(dev) for x in synth.make_batch(B, H, W, seed=rank))
        last = [None]

        def one():
            last[0] = step.step(img, cf, sdf, sal)
        units_per_step = B
    elif kind == "forward":
        net.eval()
        for p in net.parameters():
            p.requires_grad = False
        img = torch.from_numpy(synth.make_batch(B, H, W, seed=rank)[0]).to(dev)
        last = [None]

        def one():
            with torch.no_grad():
                last[0] = net.get_prediction(img)
        units_per_step = B
    else:  # sweep: one step = one 640x480 image = 1225 proposals (replicas only: every rank sweeps its own images)
        # hash weights + the peak fixtures' documented edits: a plain random-init net has empty eroded masks everywhere and the
        # peak-picking stage would be timed doing nothing (round 2's line had maps_with_peak = 0)
        spec = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.peak_edited_state_dict(spec, "base").items()}, strict=True)
        net = net.to(dev)
        net.eval()
        for p in net.parameters():
            p.requires_grad = False
        Hi, Wi = wl["image"]
        props = torch.from_numpy(anchors(Hi, Wi))
        assert props.shape[0] == wl["proposals"]
        n_img = max(1, min(4, a.steps))
        images = [torch.from_numpy(synth.blob_images(1, Hi, Wi, seed=1000 * rank + i)[0]).to(dev) for i in range(n_img)]
        counter = [0]
        peaks = [0, 0, None]
        M_head = 50 * 128 * 128

        def one():
            image = images[counter[0] % n_img]
            counter[0] += 1
            inf = {}
            peaks[0], peaks[1], peaks[2] = reasoning.sweep_proposals(net, image, props, 50, n_streams=a.sweep_streams, precision=a.sweep_precision, info=inf)
            sweep_stats[0] += inf.get("proposals", 0)
            sweep_stats[1] += inf.get("rerun", 0) or 0
        sweep_stats = [0, 0]
        units_per_step = 1

    # HIP-graph replay (unmore_amd/graphs.py): 'auto' captures the small workloads -- inference calls (cfg1 / cfg5) as one graph, train
    # steps (the reference recipe) as a chain of per-stage graphs replayed on two streams -- and leaves the large train steps eager
    # (GPU-bound, graphs.wanted).  A replayed step cannot carry per-kernel HIP events, so the dominant kernel is then timed in a
    # separate eager leg AFTER the timed region (said so in the line).
    from unmore_amd import graphs
    if kind == "train":
        step.set_graph_mode(a.graphs)
    else:
        net.set_graph_mode(a.graphs)
    pixels = (50 if kind == "sweep" else B) * H * W
    from unmore_amd.engine import WgradStream
    # (data-parallel train steps replay too where the chain-of-graphs form applies -- trainer.TrainStep: the collectives are issued between
    # the chain's graph launches; inference sweeps with world > 1 are replicas and replay as at world 1)
    graphed = ((not dist_on or kind != "train" or (graphs.STAGED and WgradStream.wanted(pixels)))
               and graphs.wanted(a.graphs, pixels, train=(kind == "train"), two_streams=WgradStream.wanted(pixels)))
    warm = a.warmup + (graphs.WARMUP_CALLS + 1 if graphed and kind != "sweep" else 0)   # two eager calls + the capturing call, untimed
    for _ in range(warm):
        one()
    barrier()
    if a.full and not graphed:
        ops.set_kernel_timer(is_head_conv)
    host_s = 0.0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        th = time.perf_counter()
        one()
        host_s += time.perf_counter() - th
    barrier()
    elapsed = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:
        # what a caller of the timed path holds after its last timed step, written before any --full leg runs the path again
        if kind == "train":
            named = [n for n, _ in net.named_parameters() if n in step.G]
            P = dict(net.named_parameters())
            outs = {"loss_terms": last[0],     # [total, center, sdf, grad, bce]
                    "params": torch.cat([P[n].detach().reshape(-1) for n in named]),     # the updated weights, named_parameters order
                    "grads": torch.cat([step.G[n].reshape(-1) for n in named])}        # the step's gradients, same order
        elif kind == "forward":
            outs = dict(last[0])
        else:
            outs = {"max_values": peaks[0], "flat_argmax": peaks[1], "deltas": peaks[2]}
        dump_outputs(a.dump_outputs, outs)
        del outs
    conv_modes, conv_ms, drained, ar_trace = [], [], [], None
    if a.full:
        if graphed:
            # separate eager leg for the roofline's kernel timing (events on the launch stream around every head-conv launch)
            ops.set_kernel_timer(is_head_conv)
            for _ in range(2):
                one()
        conv_modes = ops.kernel_timer_results_ms(with_modes=True)
        conv_ms = [m for m, _ in conv_modes]
        ops.set_kernel_timer(None)
        # the host's OWN work per step: the time to enqueue one step into an EMPTY queue.  host_s above is measured with steps queued back to
        # back: once the stream's queue is full of 30-ms kernels the launch call blocks, and that waiting is counted too (cfg2: ~190 of a
        # 226-ms step, against ~6 ms of work -- tools/enqueue_time.py)
        for _ in range(3):
            torch.cuda.synchronize()
            th = time.perf_counter()
            one()
            drained.append(time.perf_counter() - th)
        torch.cuda.synchronize()
        if dist_on and kind == "train":
            # one more, untimed step with the exchange traced: per bucket, when its all-reduce was issued and when it completed, against
            # the end of backward (parallel.BucketedAllReduce.trace_report) -- how much of the exchange hides behind backward
            # (never at the price of the line: whatever goes wrong here is reported in place of the trace)
            try:
                step.comm.trace = True
                one()
                ar_trace = step.comm.trace_report()
            except Exception as e:   # noqa: BLE001
                ar_trace = {"error": f"{type(e).__name__}: {e}"}
            step.comm.trace = False
            barrier()
    own = gather_over_ranks(elapsed)
    elapsed = max_over_ranks(elapsed)

    if rank == 0:
        fwd_gflop = forward_gflop_per_image(cfg, H, W)
        conv_flop = 2.0 * M_head * 512 * 4608
        avg_ms = sum(conv_ms) / max(len(conv_ms), 1)
        x3 = a.dtype != "bf16" and ops.get_f32_mode() == "x3"
        # fp32 parity mode: an fp32-grade product is six bf16 MFMA products (UMR_F32_X3), so the ceiling of the ALGORITHMIC f32
        # rate is the dense bf16 peak / 6 = 416.7 TFLOP/s (above the f32 MFMA's own 157.3); exact-f32 mode: the f32 MFMA peak
        peak = PEAK_BF16_TFLOPS if a.dtype == "bf16" else (PEAK_BF16_TFLOPS / 6.0 if x3 else PEAK_F32_TFLOPS)
        six_term = None
        if kind == "sweep" and x3 and a.sweep_precision == "certified":
            # the certificate-driven sweep's dominant kernel is the THREE-term plane conv of pass 1 (three bf16 MFMA products per f32
            # product: ceiling 2500 / 3); the six-term launches of pass 2 (the uncertified proposals' batches) are reported beside it
            three = [m for m, md in conv_modes if md == "x3_fast"]
            six = [m for m, md in conv_modes if md != "x3_fast"]
            if three:
                conv_ms, peak = three, PEAK_BF16_TFLOPS / 3.0
                avg_ms = sum(conv_ms) / len(conv_ms)
                if six:
                    six_term = {"launches_timed": len(six), "avg_launch_ms": sum(six) / len(six),
                                "note": "pass 2 (six-term products; batches of the uncertified proposals, the last one of an image ragged)"}
        achieved = conv_flop / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
        name = wl["name"] if a.batch is None else wl["name"].replace(f"batch={wl['batch']}", f"batch={B}")
        if a.dtype != "bf16":
            name = name.replace("bf16", a.dtype)
        metric = {"train": "images/sec (train fwd+bwd)", "forward": "images/sec (forward)", "sweep": "images/sec (inference sweep)"}[kind]
        res = {
            "metric": "images/sec (train fwd+bwd) ObjectnessNet ViT-B/16 384x384" if a.workload == "cfg2" else f"{metric} {wl['name']}",
            "value": world * units_per_step * a.steps / elapsed,
            "unit": "images/sec",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": 1e3 * elapsed / a.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": a.dtype,
            "data": "synthetic",
            "config": {"workload": name, "backbone": wl["backbone"], "reference_status": REFERENCE_STATUS[wl["backbone"]],
                       "per_gpu_batch": B, "global_batch": world * B, "image": [H, W],
                       "parallelism": (f"dp{world}" if kind == "train" else f"replicas x{world}")},
            "collective": coll,
            "cu_budget": a.cu_budget,
            "per_rank_images_per_sec": [units_per_step * a.steps / t for t in own],   # each rank's own clock between the barriers
            "peak_hbm_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
            # host time spent enqueueing one step (no synchronisation inside): what a HIP-graph replay removes
            "host_enqueue_ms_per_step": 1e3 * host_s / a.steps,
            "hip_graph": ({"mode": a.graphs, "replayed": True, "warmup_calls_untimed": warm,
                           "form": ("chain of per-stage graphs on two streams (graphs.StagedCaptured)" if kind == "train" and graphs.STAGED and WgradStream.wanted(pixels)
                                    else "one graph")}
                          if graphed else {"mode": a.graphs, "replayed": False}),
        }
        if a.full:
            res["host_enqueue_ms_per_step_queue_drained"] = 1e3 * sorted(drained)[1]
            res["host_enqueue_note"] = ("the first figure is taken with steps queued back to back and includes the launch calls' blocking on a full "
                                        "queue; the second is one step enqueued into an empty queue (median of 3, untimed leg): the host's own work")
            if graphed:
                res["hip_graph"]["roofline_timing"] = "separate eager leg of 2 steps after the timed region (no per-kernel events inside a replay)"
            res["roofline"] = {"bound": "mfma",
                               "kernel": ("umr_gemm_nt implicit-GEMM conv3x3 512->512 of the heads ("
                                          + ("per step: the centre head's forward launch + its ReLU-masked data gradient (+ the boundary-distance head's forward launch "
                                             "in 'factored' mode); the boundary-distance head is algebraic and the weight gradient is the TN kernel" if kind == "train" else "forward: the centre head's launch of every batch; the boundary-distance head runs collapsed")
                                          + (") bf16" if a.dtype == "bf16" else (") fp32-grade: f32 values as three bf16 planes, six bf16 MFMA products per "
                                                                                "f32 product; peak = 2500 / 6" if x3 else ") f32 MFMA"))),
                               "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                               "launches_timed": len(conv_ms), "avg_launch_ms": avg_ms, "flop_per_launch": conv_flop,
                               **measured_traffic(a, M_head)}
        if six_term is not None and a.full:
            res["roofline"]["six_term_launches"] = six_term
            res["roofline"]["kernel"] = res["roofline"]["kernel"].replace("six bf16 MFMA products per f32 product; peak = 2500 / 6",
                                                                          "pass 1 of the certificate-driven sweep: THREE bf16 MFMA products per f32 product; peak = 2500 / 3")
        if ar_trace is not None:
            res["allreduce_trace_rank0"] = ar_trace
        if kind == "train":
            res["config"].update({"optimizer": "Adam lr=1e-4", "loss": "l2 center + l1 sdf + l1 sdf-gradient + bce"})
            # model FLOPs (3 x forward) and the FLOPs this step actually executes: with the algebraic backward the
            # boundary-distance head's data- and weight-gradient GEMMs (2 x its forward) are not run
            head_fwd_gflop = 2.0 * H * W * (256 * 512 + 9 * 512 * 512 + 512 * 1024 + 1024) / 1e9
            skipped = 2.0 * head_fwd_gflop if net._engine().linear_head_backward == "algebraic" and not net._layouts[1]["relu"] and net._layouts[1]["final"] != "sine" else 0.0
            sdf_collapsed = net._engine()._collapse(net._layouts[1], True)
            if sdf_collapsed:
                # the default since round 6: the head's forward is its collapsed form too -- a 16-column tap GEMM
                # on the map before the final resize -- so its four convolutions are not executed in forward either
                skipped += head_fwd_gflop - 2.0 * (H / 2) * (W / 2) * 256 * 16 / 1e9
            res["sdf_head"] = ("training default 'auto': the boundary-distance head (no non-linearity before its tanh, objectness_net.py:128-135) has an "
                               "algebraic backward that reads its output only, so its forward is evaluated as one 3x3 conv 256 -> 1 on the map "
                               "before the final resize (weights stay factored; tests/test_collapsed_train_gpu.py); the four-convolution "
                               "forward is the 'alt_factored_sdf_head' leg" if sdf_collapsed else
                               "the boundary-distance head's forward runs its four convolutions (set_sdf_head_mode('factored') or a GEMM backward)")
            from unmore_amd import engine as _eng
            if _eng._COMMUTE_RESIZE:
                # 1x1 layers that run BEFORE the x2 resize that precedes them in the reference (engine._COMMUTE_RESIZE): a quarter of
                # the rows in their forward, data-gradient and weight-gradient GEMMs.  The heads' first layer (centre: all three;
                # boundary-distance: forward only when its backward is algebraic, already counted above) and the fusion blocks' out_conv
                w1 = 2.0 * H * W * 256 * 512 / 1e9
                ocv = sum(2.0 * (H / 2 ** k) * (W / 2 ** k) * 256 * 256 / 1e9 for k in (1, 2, 3, 4))
                skipped += 0.75 * (3 * w1 + (1 if skipped else 3) * w1 + 3 * ocv)
            res["train_tflops_per_gpu"] = 3 * fwd_gflop * B * a.steps / elapsed / 1e3
            res["train_tflops_note"] = "MODEL FLOPs (3 x forward formula of the reference's order of operations); executed_tflops_per_gpu counts what the step runs (algebraic head backward, 1x1 layers before the resizes)"
            res["executed_tflops_per_gpu"] = (3 * fwd_gflop - skipped) * B * a.steps / elapsed / 1e3
            res["final_loss"] = float(last[0][0].item())
        elif kind == "forward":
            res["forward_tflops_per_gpu"] = fwd_gflop * B * a.steps / elapsed / 1e3
            res["forward_tflops_note"] = ("MODEL FLOPs of the reference's order of operations; the heads' first layer and the fusion blocks' "
                                          "out_conv run before the x2 resize that precedes them (a quarter of the rows): ~2 % fewer executed")
        else:
            res["crops_per_sec"] = world * wl["proposals"] * a.steps / elapsed
            res["config"].update({"proposals_per_image": wl["proposals"], "crop": [128, 128], "crops_per_batch": 50,
                                  "source_image": list(wl["image"]),
                                  "stages": "crop+resize, ObjectnessNet maps, centre peak picking, boundary box deltas"})
            res["est_minutes_for_5000_images"] = 5000.0 / res["value"] / 60.0
            if a.full and a.sweep_streams > 1:
                res["roofline"]["note"] = ("batches on different HIP streams share the chip: a conv launch is timed while kernels of the other "
                                           "streams run beside it, so `achieved` is a lower bound of the kernel alone (--sweep-streams 1)")
            res["maps_with_peak"] = int((peaks[0] > 0).sum().item())
            res["config"]["streams"] = a.sweep_streams
            certified_mode = a.dtype == "fp32" and a.sweep_precision == "certified" and ops.get_f32_mode() == "x3"
            res["sweep_precision"] = ({"mode": "certified", "rerun_fraction": sweep_stats[1] / max(sweep_stats[0], 1),
                                       "note": "pass 1: every proposal with three-term fp32 products (maps within ~4e-5 of the six-term ones) + the device-side "
                                               "argmax certificate at eps = 2e-4 (csrc/reasoning.hip::center_peaks_cert_kernel); pass 2: the uncertified "
                                               "proposals again with six-term products; rerun_fraction = their share over all sweeps of this run "
                                               "(warm-up included).  Peak indices equal the full six-term sweep's on every proposal "
                                               "(alt_fp32_full_precision.peak_index_differs_from_headline; tests/test_certified_sweep_gpu.py)"}
                                      if certified_mode else {"mode": "full"})
        hip_peaks = None
        if kind == "sweep":
            res["maps_with_peak_share"] = res["maps_with_peak"] / wl["proposals"]
        if a.full and not dist_on and kind == "sweep" and not a.no_alt:
            def timed_sweeps(n):
                one()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(n):
                    one()
                torch.cuda.synchronize()
                return (time.perf_counter() - t1) / n
            if a.dtype == "fp32":
                # the peaks the CPU leg re-derives: image 0, proposals SWEEP_CHECK, in the headline (fp32 parity) mode
                mx0, am0, _ = reasoning.sweep_proposals(net, images[0], props, 50, n_streams=a.sweep_streams, precision=a.sweep_precision)
                hip_peaks = (mx0.cpu(), am0.cpu())
                if a.sweep_precision == "certified":
                    # beside the headline: EVERY proposal with six-term products (the headline of rounds 2-5), and its peak indices
                    saved = a.sweep_precision
                    a.sweep_precision = "full"
                    try:
                        dt6 = timed_sweeps(2)
                        mx6, am6, _ = reasoning.sweep_proposals(net, images[0], props, 50, n_streams=a.sweep_streams, precision="full")
                    finally:
                        a.sweep_precision = saved
                    res["alt_fp32_full_precision"] = {"value": 1.0 / dt6, "unit": "images/sec", "crops_per_sec": wl["proposals"] / dt6,
                                                      "peak_index_differs_from_headline": int((am6 != am0).sum().item()),
                                                      "max_abs_amax_difference_vs_headline": float((mx6 - mx0).abs().max().item()),
                                                      "note": "sweep_proposals(precision='full'): six-term fp32-grade products for every proposal, no certificate"}
                # beside the headline, never `value`: the opt-in three-term plane products (UMR_F32_X3_FAST: products to 2^-16, half
                # the matrix work) with what they cost in the maps and in the peak indices, measured on the same image
                saved_prec, a.sweep_precision = a.sweep_precision, "full"     # the legs below time ONE arithmetic mode each
                ops.set_f32_mode("x3_fast")
                try:
                    dtf = timed_sweeps(2)
                    mxf, amf, _ = reasoning.sweep_proposals(net, images[0], props, 50, n_streams=a.sweep_streams)
                    crops_chk, _ = reasoning.crop_resize(images[0], props[SWEEP_CHECK[0]:SWEEP_CHECK[1]], 128)
                    with torch.no_grad():
                        pf = net.get_prediction(crops_chk)
                    ops.set_f32_mode("x3")
                    with torch.no_grad():
                        p6 = net.get_prediction(crops_chk)
                finally:
                    ops.set_f32_mode("x3")
                res["alt_fp32_3term"] = {"value": 1.0 / dtf, "unit": "images/sec", "crops_per_sec": wl["proposals"] / dtf,
                                         "peak_index_differs_from_6term": int((amf != am0).sum().item()),
                                         "max_abs_map_difference_vs_6term": float(max((pf[k] - p6[k]).abs().max().item() for k in ("center_fields", "sdf_maps"))),
                                         "note": "opt-in umr_set_f32_mode(UMR_F32_X3_FAST): three instead of six bf16 products per f32 product in the heads' "
                                                 "plane GEMMs (2^-16 per product); not the headline"}
                # the other way round (A/B of the inference default): the boundary-distance head as the reference's four convolutions
                # instead of its collapsed form (one 3x3 conv 256 -> 1), same image, all 1225 proposals compared
                net.set_sdf_head_mode("factored")
                dtF = timed_sweeps(2)
                mxF, amF, _ = reasoning.sweep_proposals(net, images[0], props, 50, n_streams=a.sweep_streams)
                with torch.no_grad():
                    pF = net.get_prediction(crops_chk)
                net.set_sdf_head_mode("auto")
                res["alt_fp32_factored_sdf_head"] = {"value": 1.0 / dtF, "unit": "images/sec", "crops_per_sec": wl["proposals"] / dtF,
                                                     "maps_with_peak": int((mxF > 0).sum().item()),
                                                     "peak_index_differs_from_headline": int((amF != am0).sum().item()),
                                                     "max_abs_map_difference_vs_headline": float(max((pF[k] - p6[k]).abs().max().item() for k in ("center_fields", "sdf_maps"))),
                                                     "note": "set_sdf_head_mode('factored'): the head's four convolutions as the reference runs them; the headline is "
                                                             "the inference default ('auto': collapsed under no_grad, qualified in tests/test_collapsed_head_gpu.py)"}
                # beside the headline: the same sweep with bf16 storage (no bit-exact-peak claim) ...
                net.set_compute_dtype(torch.bfloat16)
                dt2 = timed_sweeps(2)
                mxb, amb, _ = reasoning.sweep_proposals(net, images[0], props, 50, n_streams=a.sweep_streams)
                res["alt_bf16"] = {"value": 1.0 / dt2, "unit": "images/sec", "crops_per_sec": wl["proposals"] / dt2,
                                   "maps_with_peak": int((mxb > 0).sum().item()),
                                   "peak_index_differs_from_fp32_mode": int((amb != am0).sum().item()),
                                   "note": "bf16 storage / bf16 MFMA: throughput mode, maps within ~3e-2 of the reference, peak indices NOT claimed"}
                # ... and bf16 with the boundary-distance head's four convolutions
                net.set_sdf_head_mode("factored")
                dt3 = timed_sweeps(2)
                net.set_sdf_head_mode("auto")
                res["alt_bf16_factored_sdf_head"] = {"value": 1.0 / dt3, "unit": "images/sec", "crops_per_sec": wl["proposals"] / dt3,
                                                     "note": "bf16 with set_sdf_head_mode('factored')"}
                net.set_compute_dtype(dt)
                a.sweep_precision = saved_prec
            else:
                net.set_compute_dtype(torch.float32)
                dt2 = timed_sweeps(1)
                net.set_compute_dtype(dt)
                res["alt_fp32_parity_mode"] = {"value": 1.0 / dt2, "unit": "images/sec", "crops_per_sec": wl["proposals"] / dt2,
                                               "note": "fp32 storage, fp32-grade products (UMR_F32_X3): the 1e-4 maps / bit-exact-peaks mode; the default --dtype of this workload"}
        if kind != "train":
            res["sdf_head"] = ("inference default 'auto': the boundary-distance head (no non-linearity before its tanh, objectness_net.py:128-135) "
                               "evaluated as one 3x3 conv 256 -> 1 on the map before the final resize; 'factored' leg beside it")
        if a.full and not dist_on and kind == "forward" and not a.no_alt:
            # the same call with the boundary-distance head as the reference's four convolutions (A/B of the inference default)
            net.set_sdf_head_mode("factored")
            for _ in range(graphs.WARMUP_CALLS + 2):
                one()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(a.steps):
                one()
            torch.cuda.synchronize()
            dtf = (time.perf_counter() - t1) / a.steps
            net.set_sdf_head_mode("auto")
            res["alt_factored_sdf_head"] = {"value": B / dtf, "unit": "images/sec", "ms_per_step": 1e3 * dtf,
                                            "note": "set_sdf_head_mode('factored'): the head's four convolutions as the reference runs them"}
        if a.full and not dist_on and kind == "train" and a.workload == "cfg2" and not a.no_alt:
            # outside the timed region, reported BESIDE the headline: the same step with the boundary-distance head in its other forms
            # (identical function and gradients up to rounding, tests/test_train_gpu.py::
            # test_collapsed_sdf_head_equals_factored, tests/test_collapsed_train_gpu.py)
            del step

            def alt_leg(note):
                st = TrainStep(net, lr=1e-4, lr_milestones=(10000, 20000), lr_gamma=0.1)
                for _ in range(2):
                    st.step(img, cf, sdf, sal)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(3):
                    st.step(img, cf, sdf, sal)
                torch.cuda.synchronize()
                d = (time.perf_counter() - t1) / 3
                return {"value": B / d, "unit": "images/sec", "ms_per_step": 1e3 * d, "note": note}
            # (1) the head's forward as the reference's four convolutions (rounds 2-5's headline form; backward algebraic as in `value`)
            net.set_sdf_head_mode("factored")
            res["alt_factored_sdf_head"] = alt_leg("set_sdf_head_mode('factored'): the head's four convolutions in forward as the reference runs them "
                                                   "(their 512/512/1024-channel maps are not read by the algebraic backward); the headline of rounds 2-5")
            # (2) and its backward as layer-by-layer GEMMs too (the round-1 form)
            net.set_linear_head_backward("gemm")
            res["alt_gemm_backward_sdf_head"] = alt_leg("factored forward + boundary-distance head backward as layer-by-layer GEMMs (the reference's own schedule of operations)")
            net.set_linear_head_backward("algebraic")
            net.set_sdf_head_mode("auto")
        if a.full and not dist_on and not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(wl, hip_peaks)
        print(json.dumps(res), flush=True)
    if dist_on:
        barrier()
        dist.destroy_process_group()
    return 0


def rehearse(a, wl, world, rank, coll, barrier, max_over_ranks, gather_over_ranks):
    """Multi-process plumbing alone (CPU tensors): what bench.py does around the model for N > 1."""
    import torch
    import torch.distributed as dist
    from argparse import Namespace
    from unmore_amd.objectness_net import ObjectnessNet
    from unmore_amd.parallel import BucketedAllReduce
    # the step's real exchange: the flat gradient buffer of the workload's model (parameters that receive gradients, 256-byte
    # aligned views) in its backward-completion buckets -- 115.4 M elements in 16 buckets for ViT-B (unmore_amd/trainer.py); the
    # module only HOLDS parameters, nothing is computed
    from unmore_amd.trainer import flat_layout
    _, bounds, _ = flat_layout(ObjectnessNet("cpu", wl["H"], wl["backbone"], Namespace(use_bg_sdf=True, sdf_activation="tanh")))
    n, nb = bounds[-1], len(bounds) - 1
    flat = torch.full((n,), float(rank + 1))
    wire = a.dp_wire == "bf16"
    comm = BucketedAllReduce(flat, bounds, wire_dtype=(torch.bfloat16 if wire else None))
    for _ in range(a.warmup):
        for k in range(nb):
            comm.ready(k)
        comm.finish()
    flat.fill_(float(rank + 1))
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        for k in range(nb):
            comm.ready(k)
        scale = comm.finish()
    barrier()
    own = gather_over_ranks(time.perf_counter() - t0)
    elapsed = max_over_ranks(own[rank] if world > 1 else own[0])
    if wire:     # the bf16 wire exchanges means (1/world before the rounding): (world + 1) / 2 after the first step and ever after -- exact in bf16
        expect = (world + 1) / 2.0
        ok = bool(torch.all(flat == expect)) and scale == 1.0
    else:
        expect = float(sum(range(1, world + 1))) * (world ** (a.steps - 1))
        ok = bool(torch.all(flat == expect)) and scale == 1.0 / world
    if rank == 0:
        print(json.dumps({"rehearsal": True, "metric": "distributed plumbing only (no model)", "value": None, "n_gpus": world, "steps": a.steps,
                          "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps, "collective": coll, "allreduce_elements": n, "allreduce_buckets": nb,
                          "allreduce_correct": ok, "per_rank_ms_per_step": [1e3 * t / a.steps for t in own], "config": {"workload": wl["name"], "parallelism": f"dp{world}"}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: the workload's)")
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp32"],
                    help="default: bf16 for the train / forward workloads (BASELINE configs[0..3]); fp32 for cfg5 -- configs[4] asks for peak "
                         "picking bit-exact vs the CPU, which only the fp32 parity mode claims (bf16 is reported beside it)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL over xGMI; gloo = rehearsal transport (ranks may share a GPU)")
    ap.add_argument("--rehearse", action="store_true", help="CPU-only: run the multi-process plumbing without the model")
    ap.add_argument("--sweep-streams", type=int, default=3, help="cfg5: HIP streams the independent 50-crop batches are dealt to")
    ap.add_argument("--sweep-precision", default="certified", choices=["certified", "full"],
                    help="cfg5, fp32: 'certified' (default) = three-term products + device-side argmax certificate, six-term re-run of the "
                         "uncertified proposals (unmore_amd/reasoning.py::sweep_proposals); 'full' = six-term products for every proposal")
    ap.add_argument("--launch-timeout", type=float, default=1500.0, help="plain --gpus N launch: overall deadline in seconds, counted from the launch")
    ap.add_argument("--fail-rank", type=int, default=None, help=argparse.SUPPRESS)   # launcher test hook
    ap.add_argument("--graphs", default="auto", choices=["auto", "on", "off"],
                    help="HIP-graph replay: auto = small inference workloads only (B*H*W <= 2^20 pixels), on = also train steps")
    ap.add_argument("--dp-wire", default="f32", choices=["f32", "bf16"],
                    help="data-parallel gradient exchange: f32 buckets as they are (default) or bf16 copies (half the bytes per link; "
                         "unmore_amd/parallel.py, DESIGN.md section 6)")
    ap.add_argument("--cu-budget", type=int, default=0,
                    help="CUs the persistent GEMM grids occupy (umr_set_cu_budget; 0 = all): leaves the rest to RCCL's kernels when world > 1")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the roofline kernel timing, the drained-queue enqueue time, the traced gradient exchange "
                         "(N > 1), the non-headline alt_* legs and the CPU baseline; a plain run times the headline steps only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-alt", action="store_true", help="--full without the extra (non-headline) factored-sdf-head / GEMM-backward measurements")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32 / float64, "
                         "rank 0, at most 64 MB in all: larger arrays as a fixed seeded sample)")
    a = ap.parse_args()
    if a.dtype is None:
        a.dtype = "fp32" if WORKLOADS[a.workload]["kind"] == "sweep" else "bf16"
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(a.gpus, a.launch_timeout)
    return run_rank(a)


if __name__ == "__main__":
    sys.exit(main())
