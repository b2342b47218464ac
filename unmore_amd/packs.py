"""Kernel-layout copies of parameters: what both engine modules need and neither schedule owns.

PackCache keeps the repacked weights per parameter version (ParamGroup: a pack derived from several parameters); the _pack_* helpers
turn the reference's PyTorch layouts into the layouts the GEMM kernels read, each as ONE permute / cast that PackCache.refresh can
replay.  engine.py re-exports these names (tests and tools address them as engine.PackCache, engine._pack_linear_t, ...).
"""
import torch

from . import _lib as L
from . import graphs
from . import ops

_ACT = {None: L.ACT_NONE, "tanh": L.ACT_TANH, "sine": ops.ACT_SINE}    # a head's output activation (objectness_net.py:117,133)


class ParamGroup:
    """Several parameters seen by PackCache.get as one: the key of a pack derived from all of them (the collapsed head's weight
    algebra reads eight tensors) -- its version is the tuple of theirs, so a change of any one misses."""

    def __init__(self, params):
        self.ps = tuple(params)
        self.is_cuda, self.device = self.ps[0].is_cuda, self.ps[0].device

    @property
    def _version(self):
        return tuple(p._version for p in self.ps)

    def data_ptr(self):
        return tuple(p.data_ptr() for p in self.ps)


class PackCache:
    """Kernel-layout copies of parameters, rebuilt when the parameter changes.

    Stream-safe: an entry is built by kernels enqueued on whatever stream touches it first and is published to this host-side
    dict at once, so a consumer on ANOTHER stream (reasoning.sweep_proposals deals batches to several streams) could launch
    a GEMM that reads the packed buffer before the pack kernel has run.  Every entry therefore carries an event recorded
    right after its build; a hit from a stream that has not yet ordered itself after that event waits on it first (once per
    stream and entry -- afterwards the stream's own order covers it)."""

    def __init__(self):
        self._c = {}           # key -> [version, value, event, synced streams, recipe, param]: replayable packs
        self._o = {}           # same without a recipe: rebuilt lazily after refresh()
        self._replay = {}      # tag -> (launcher, keys) of a batched refresh (None: all entries), built on first use
        # A captured graph holds the ADDRESSES of the copies it read: gen_c counts changes of the replayable set (and of the batched
        # refresh's table), gen_o changes of the rest.  A capture depends on gen_o only if it read such an entry that it did not
        # build itself (a capture rebuilds its own on every replay): generation(store)
        self.gen_c = 0
        self.gen_o = 0
        self._epoch = None     # (event, synced streams) of the last refresh that ran inside a graph replay (graphs.py)

    def get(self, key, param, build, recipe_fn=None):
        """recipe_fn(recorded launches, value) -> replay recipe or None: for packs whose replayable form is not the launch that
        built them (the bf16-plane weights: built as f32 pack + split, refreshed as one permute straight into planes)"""
        ver = (param._version, param.data_ptr())
        hit = self._c.get(key) or self._o.get(key)
        cap = graphs.capturing()
        sid = ops._stream_id(param.device.index) if param.is_cuda else None    # raw handle: no Stream object on the hit path
        if hit is not None and hit[0] == ver:
            if cap and key in self._o and hit[6] is not graphs.capture_store():
                graphs.capture_store()["hit_o"] = True
            # (inside a capture nothing from before it is pending -- graphs.Captured synchronises first -- and an event wait on
            # work outside the capture must not be recorded into it)
            if sid is not None and not cap:
                if hit[2] is not None and sid not in hit[3]:
                    torch.cuda.current_stream(param.device).wait_event(hit[2])
                    hit[3].add(sid)
                if self._epoch is not None and sid not in self._epoch[1]:
                    torch.cuda.current_stream(param.device).wait_event(self._epoch[0])
                    self._epoch[1].add(sid)
            return hit[1]
        st = torch.cuda.current_stream(param.device) if param.is_cuda else None
        # record what the build launches: a pack that is exactly ONE permute / cast into the returned tensor can be replayed by
        # refresh() (every pack helper below is); anything else is rebuilt lazily after a refresh
        rec = []
        prev, ops._pack_recorder = ops._pack_recorder, rec
        try:
            val = build()
        finally:
            ops._pack_recorder = prev
        # replayable only if the recorded source IS the parameter's storage: a pack helper that had to make a temporary copy first
        # (reshape of a non-contiguous parameter) would be re-packed from that stale temporary forever
        if recipe_fn is not None:
            recipe = recipe_fn(rec, val)
            if recipe is not None and recipe[0].untyped_storage().data_ptr() != param.untyped_storage().data_ptr():
                recipe = None
        else:
            recipe = rec[0] if (len(rec) == 1 and torch.is_tensor(val) and rec[0][1].data_ptr() == val.data_ptr()
                                and rec[0][0].untyped_storage().data_ptr() == param.untyped_storage().data_ptr()) else None
        ev = None
        if st is not None and not cap:
            ev = torch.cuda.Event()
            ev.record(st)
        entry = [ver, val, ev, {sid}, recipe, param, (graphs.capture_store() if cap else None)]
        if self._c.pop(key, None) is not None:
            self._replay = {}         # the batched refreshes were built over the dropped entry
            self.gen_c += 1
        if self._o.pop(key, None) is not None:
            self.gen_o += 1
        if recipe is not None and st is not None:
            self._c[key] = entry
            self._replay = {}
            self.gen_c += 1
        else:
            self._o[key] = entry
            self.gen_o += 1
        return val

    def generation(self, store=None):
        """validity stamp of a capture whose scratch dict is `store` (graphs.Captured)"""
        return (self.gen_c, self.gen_o if (store is None or store.get("hit_o")) else None)

    def clear(self):
        self._c.clear()
        self._o.clear()
        self._replay = {}
        self._epoch = None
        self.gen_c += 1
        self.gen_o += 1

    def purge_capture(self, store):
        """A HIP-graph capture whose scratch dict is `store` FAILED: the packs it built were only recorded, never executed -- their
        buffers (in the capture's private pool) hold nothing, yet they sit in the cache under the parameters' current versions.
        Drop them, so the eager path that takes over re-packs (graphs.Captured calls this from its failure path)."""
        dead_c = [k for k, e in self._c.items() if e[6] is store]
        dead_o = [k for k, e in self._o.items() if e[6] is store]
        for k in dead_c:
            del self._c[k]
        for k in dead_o:
            del self._o[k]
        if dead_c:
            self._replay = {}
            self.gen_c += 1
        if dead_o:
            self.gen_o += 1
        return len(dead_c) + len(dead_o)

    def refresh(self, tag=None, select=None):
        """The parameters were updated IN PLACE by a kernel torch does not see (TrainStep's Adam launch): re-run every pack into
        its existing destination in ONE launch (umr_permute4_batched) instead of dropping the copies and re-packing ~180
        weights one launch each during the next step.  Entries that are not a single permute are dropped (rebuilt lazily).
        tag / select(key): refresh only the entries select() accepts (one launch per tag: TrainStep updates and refreshes stage
        by stage, beside the rest of backward); the caller ends the round of partial refreshes with refresh_done()."""
        if tag is None:
            self.refresh_done()
        if not self._c:
            return
        if tag not in self._replay:
            assert not graphs.capturing(), "PackCache.refresh: the batched refresh must be built before a capture (warm-up steps)"
            keys = [k for k in self._c if select is None or select(k)]
            self._replay[tag] = (ops.permute4_batched([self._c[k][4] for k in keys]) if keys else None, keys)
        launch, keys = self._replay[tag]
        if launch is None:
            return
        if any(self._c[k][5].data_ptr() != self._c[k][0][1] for k in keys):   # a parameter's storage moved: the recipes are stale
            self.clear()
            return
        launch()
        if graphs.capturing():
            return                     # the replaying caller publishes the refresh with refreshed_by_replay()
        st = torch.cuda.current_stream(self._c[keys[0]][5].device)
        ev = torch.cuda.Event()
        ev.record(st)
        for k in keys:
            e = self._c[k]
            e[0] = (e[5]._version, e[5].data_ptr())
            e[2], e[3] = ev, {st.cuda_stream}

    def adam_and_refresh(self, tag, select, stage_params, lo, hi, bufs, hyper):
        """Optimizer step of the flat-buffer slice [lo, hi) AND the refresh of its packed copies, with the copies of its Linear
        weights written by the optimizer launch itself (ops.adam_pack / umr_adam_pack_step: the refresh pass that re-read those f32
        weights is gone; the other packs of the stage -- conv layouts, plane forms -- keep the batched permute).
        stage_params: [(name, element offset, numel, shape)] of the slice in buffer order; bufs = (flat p, g, m, v); hyper: device
        scalars of umr_adam_set_hyper.  Returns False (nothing launched) when no weight of the stage has a bf16 [N,K] / [K,N] copy
        -- the caller then runs the two-launch form.  Bit-identical to it (tests/test_train_gpu.py)."""
        rk = ("adam", tag)
        if rk not in self._replay:
            assert not graphs.capturing(), "PackCache.adam_and_refresh: the tables must be built before a capture (warm-up steps)"
            keys = [k for k in self._c if select is None or select(k)]
            by_name = {}
            for k in keys:
                by_name.setdefault(k[0], {})[k[1]] = k
            flat_p, flat_g, flat_m, flat_v = bufs
            entries, fused, cur = [], set(), lo
            for name, off, numel, shape in stage_params:
                kinds = by_name.get(name, {})
                ok = (len(shape) == 2 and shape[0] % 8 == 0 and shape[1] % 4 == 0 and off % 4 == 0 and kinds and set(kinds) <= {"lin", "lin_t"}
                      and all(torch.is_tensor(self._c[k][1]) and self._c[k][1].dtype == torch.bfloat16 and self._c[k][1].is_contiguous()
                              for k in kinds.values()))
                if ok:
                    dl = self._c[kinds["lin"]][1] if "lin" in kinds else None
                    dt_ = self._c[kinds["lin_t"]][1] if "lin_t" in kinds else None
                    ok = (dl is None or tuple(dl.shape) == tuple(shape)) and (dt_ is None or tuple(dt_.shape) == (shape[1], shape[0]))
                if not ok:
                    continue
                if cur < off:
                    entries.append(("plain",) + tuple(b[cur:off] for b in bufs))
                entries.append(("weight",) + tuple(b[off:off + numel].view(shape) for b in bufs) + (dl, dt_))
                fused.update(kinds.values())
                cur = off + numel
            if not fused:
                self._replay[rk] = None
            else:
                if cur < hi:
                    entries.append(("plain",) + tuple(b[cur:hi] for b in bufs))
                rest = [k for k in keys if k not in fused]
                self._replay[rk] = (ops.adam_pack(entries, hyper), ops.permute4_batched([self._c[k][4] for k in rest]) if rest else None, keys)
        rec = self._replay[rk]
        if rec is None:
            return False
        launch_adam, launch_rest, keys = rec
        if any(self._c[k][5].data_ptr() != self._c[k][0][1] for k in keys):   # a parameter's storage moved: the tables are stale
            self.clear()
            return False
        launch_adam()
        if launch_rest is not None:
            launch_rest()
        if graphs.capturing():
            return True                # the replaying caller publishes the refresh with refreshed_by_replay()
        st = torch.cuda.current_stream(self._c[keys[0]][5].device)
        ev = torch.cuda.Event()
        ev.record(st)
        for k in keys:
            e = self._c[k]
            e[0] = (e[5]._version, e[5].data_ptr())
            e[2], e[3] = ev, {st.cuda_stream}
        return True

    def refresh_done(self):
        """after the last (partial) refresh of a round: the copies that cannot be replayed are dropped (rebuilt on next use).
        Inside a capture, entries the capture built itself go silently (each of its replays rebuilds them); every OTHER dropped entry
        -- e.g. the collapsed head's weights an evaluation call cached between a TrainStep's warm-up and its capturing step -- counts
        as a change of the set, so an inference capture that read it (hit_o) is invalidated instead of replaying from freed memory."""
        if self._o:
            cur = graphs.capture_store() if graphs.capturing() else None
            foreign = cur is None or any(e[6] is not cur for e in self._o.values())
            self._o.clear()
            if foreign:
                self.gen_o += 1

    def synced_with(self, stream):
        """`stream` has waited for the stream(s) the refreshes ran on (a join): its later launches need no per-entry event wait"""
        sid = stream.cuda_stream
        for e in self._c.values():
            e[3].add(sid)

    def refreshed_by_replay(self, device):
        """A graph replay on the current stream has just re-run the optimizer step and the refresh: a consumer on another stream
        orders itself after it (one event for the whole cache instead of one per entry).  The replay updated the parameters on
        the device without running this class's host code, so what refresh_done() does after an eager step is done here: EVERY copy
        that cannot be replayed is stale in this host-side dict now and is dropped -- those built outside a capture (the collapsed head's
        weights an evaluation call cached between two training steps) and those an inference capture built inside itself: that capture
        holds the addresses and rewrites them on each of its replays, but a cache HIT by anybody else (an eager call of another shape,
        a second capture) would read what the first graph's LAST replay wrote, i.e. weights one or more steps old (round-5 advisor)."""
        if self._o:
            self._o.clear()
            self.gen_o += 1
        st = torch.cuda.current_stream(device)
        ev = torch.cuda.Event()
        ev.record(st)
        self._epoch = (ev, {st.cuda_stream})


def _pack_linear(w, dt):  # [N,K] -> [N,K] T
    return ops.cast(w.detach().reshape(w.shape[0], -1), dt)


def _pack_linear_t(w, dt):  # [N,K] (possibly strided rows) or [N,...] contiguous -> [K,N] T
    w2d = w.detach().reshape(w.shape[0], -1)
    N, K = w2d.shape
    out = torch.empty((K, N), dtype=dt, device=w2d.device)
    return ops.permute4(w2d, out, (1, 1, K, N), (0, 0, w2d.stride(1), w2d.stride(0)), src_offset=0)


def _pack_conv3(w, dt):  # [co,ci,3,3] -> [co][ky][kx][ci]
    co, ci = w.shape[0], w.shape[1]
    st = w.stride()
    out = torch.empty((co, 9 * ci), dtype=dt, device=w.device)
    return ops.permute4(w.detach(), out, (co, 3, 3, ci), (st[0], st[2], st[3], st[1]))


def _pack_conv3_dgrad(w, dt):  # [co,ci,3,3] -> [ci][2-ky][2-kx][co]
    co, ci = w.shape[0], w.shape[1]
    st = w.stride()
    out = torch.empty((ci, 9 * co), dtype=dt, device=w.device)
    return ops.permute4(w.detach(), out, (ci, 3, 3, co), (st[1], -st[2], -st[3], st[0]), src_offset=2 * st[2] + 2 * st[3])


def _unpack_conv3_grad(dwp, grad_out):  # [co][ky][kx][ci] f32 -> [co,ci,3,3] f32
    co, ci = grad_out.shape[0], grad_out.shape[1]
    return ops.permute4(dwp, grad_out, (co, ci, 3, 3), (9 * ci, 1, 3 * ci, ci))


def _pack_convT(w, dt):  # ConvTranspose2d [ci,co,s,s] -> [(i,j,co)][ci]
    ci, co, s, _ = w.shape
    st = w.stride()
    out = torch.empty((s * s * co, ci), dtype=dt, device=w.device)
    return ops.permute4(w.detach(), out, (s, s, co, ci), (st[2], st[3], st[1], st[0]))


def _pack_convT_dgrad(w, dt):  # -> [ci][(i,j,co)]
    ci, co, s, _ = w.shape
    st = w.stride()
    out = torch.empty((ci, s * s * co), dtype=dt, device=w.device)
    return ops.permute4(w.detach(), out, (ci, s, s, co), (st[0], st[2], st[3], st[1]))


def _rep_bias(b, reps):
    out = torch.empty(reps * b.numel(), dtype=torch.float32, device=b.device)
    return ops.permute4(b.detach(), out, (1, 1, reps, b.numel()), (0, 0, 0, 1))


# kind -> builder(parameter, compute type) of the layouts Engine._w, Engine._wx3 and the conv heads ask for by name
BUILDERS = {"lin": _pack_linear, "lin_t": _pack_linear_t, "c3": _pack_conv3, "c3_d": _pack_conv3_dgrad, "ct": _pack_convT,
            "ct_d": _pack_convT_dgrad}
