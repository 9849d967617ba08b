"""Host bookkeeping of ``model.Trainer``'s step that spans its segments.  ``GradSync``: what happens to an optimizer key once its
backward segment is complete, the join at the end of the backward pass, which keys have stepped.  ``StepGraph``: the step captured
as a sequence of HIP graphs and replayed.  The order of the calls in ``Trainer._step_impl`` is still the order of the launches."""
import contextlib
import weakref
from collections import deque

import torch

from . import dist as D, ops, switches as SW, tps as TPS

JOIN_TIMING = SW.flag("UPS_JOIN_TIMING")
EARLY_ADAM = SW.flag("UPS_EARLY_ADAM")    # test switch: a single rank queues each key's Adam behind its weight gradients


class GradSync(object):
    """One per Trainer (``trainer.sync``).  ``stepped``: the keys whose Adam step of the RUNNING eager step has been enqueued
    (``Trainer._adam`` adds each as it steps): the early ones of ``segment_done``, then those of ``finish``'s loop.  ONE set:
    an early Adam only runs with ``graph_lr is None`` and therefore always through the branch of ``_adam`` that records."""

    def __init__(self, trainer):
        self.tr = weakref.proxy(trainer)        # (no reference cycle: a dropped trainer is freed at once, not by a later collection)
        self.head_hooked, self.head_inflight = False, None      # hook_head: installed; (offset, handle) of the slice under way
        # bounded aids for short runs: (events, marks) per timed data-parallel wait (dp_wait_ms); event pairs around the two joins (join)
        self.dp_wait_events, self.join_events, self.tail_events = deque(maxlen=64), deque(maxlen=256), deque(maxlen=256)
        self.begin(None)

    def begin(self, graph_lr):
        """graph_lr: device scalar holding lr_t (HIP-graph mode, eager warm-up steps included), else None.  ``handles``: the step's
        all-reduce work handles; ``marks``: (key, bytes) per handle, in launch order."""
        self.graph_lr, self.stepped, self.handles, self.marks = graph_lr, set(), [], []

    def abort(self):
        """The step raised: the sorted keys that have stepped (early on the side stream AND in a partly run final loop); a clean slate."""
        done, self.head_inflight = sorted(self.stepped), None
        self.begin(None)
        ops.Streams.master_busy.clear()
        return done

    def join(self, which, names=("wgrad", "aux")):
        """``ops.Streams.join``; under JOIN_TIMING in an eager step between two timing events, kept in ``<which>_events``."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if JOIN_TIMING and self.graph_lr is None else None
        if ev:
            ev[0].record()
        ops.Streams.join(self.tr.device, names=names)
        if ev:
            ev[1].record()
            getattr(self, which + "_events").append(ev)

    def _reduce_from(self, current=True):
        """The context a bucket's all-reduce is enqueued in: the weight-gradient stream's position (torch's process group orders its
        stream behind the stream current at the call), so that the LAUNCHING stream need not wait for the segment's weight gradients
        (DESIGN section 7).  Without side streams it joins that stream instead."""
        if ops.Streams.enabled:
            return torch.cuda.stream(ops.Streams.wgrad_behind(self.tr.device, current=current))
        ops.Streams.join(self.tr.device, names=("wgrad",))
        return contextlib.nullcontext()

    def hook_head(self):
        """The 1x1 head of encoder_0 (258 x 33152 weights = 34 of the key's 54.6 MB) is the FIRST weight gradient of the last backward
        segment: its slice of the flat bucket starts its all-reduce as soon as it has been enqueued, so only the remaining 20 MB
        follow the end of the backward pass.  (Called before that segment: layers exist once the first forward has run.)"""
        tr = self.tr
        if self.head_hooked or not (tr.world_size > 1 or D.FORCE_COLLECTIVES):
            return
        grp, size = tr.model.bank.groups["encoder_0"], lambda n: tr.model.bank.params[n].numel()
        prefix = max((n for n in grp["names"] if n.endswith("/V")), key=lambda n: int(n.split("conv2d_")[1].split("/")[0]))[:-2]
        first = [n.startswith(prefix + "/") for n in grp["names"]].index(True)
        off = sum(size(n) for n in grp["names"][:first])
        assert off + sum(size(n) for n in grp["names"] if n.startswith(prefix + "/")) == grp["flat"]["g"].numel(), "the head's variables must close the flat bucket"

        def launch():
            if self.head_inflight is None and not (tr.graph is not None and tr.graph.capturing):    # (capture: the whole bucket at its boundary)
                with self._reduce_from(current=False):      # behind the head's weight gradient on ITS stream: the hook runs right after it
                    self.head_inflight = (off, D.allreduce_bucket(grp["flat"]["g"][off:], tr.world_size, tr.process_group))

        for key, lay in tr.model.nets.layers.items():
            if key[0] == prefix:
                lay.after_wgrad = launch
        self.head_hooked = True

    def segment_done(self, keys):
        """Called when the backward segment of these optimizer keys is complete: their weight gradients (side stream) are joined and
        each key's flat bucket starts its RCCL all-reduce (sum; 1/world is folded into Adam), overlapping the segments still to run."""
        tr = self.tr
        if not keys:
            return
        if tr.graph is not None and tr.graph.capturing:      # graph capture: under data parallelism a segment boundary, else nothing
            if tr.world_size > 1 or D.FORCE_COLLECTIVES:
                tr.graph.boundary("grads", list(keys))
            return
        if tr.world_size == 1 and not D.FORCE_COLLECTIVES:
            # a single rank has nothing to reduce: the launching stream need not wait for the weight-gradient stream here (it would idle
            # whenever that stream lags); both meet before the end of the step (finish).  The tensors the side stream reads stay
            # referenced until then (ops.Streams.keep).  The keys' Adam updates are queued right BEHIND their weight gradients on that
            # stream (EARLY_ADAM): the fp32 master weights are not read again this step -- every convolution works on the converted
            # copies, refreshed once all keys have stepped -- so the 0.9 GB optimizer stream runs in the shadow of the remaining
            # backward pass instead of on an otherwise empty chip at the end.
            if EARLY_ADAM and ops.Streams.enabled and self.graph_lr is None:
                side = ops.Streams.wgrad_behind(tr.device, create=True)     # (critics: their gradients were taken on "aux", joined by now)
                with torch.cuda.stream(side):
                    tr._adam(keys, None)
                    ev = side.record_event()
                # a converted-weight cache entry created later in this step (a new (dtype, size) instance, the depth-to-space or
                # fp8 copies) reads the fp32 master: it must see the finished update, not race with it (ops.WeightCopy._wait_master)
                ops.Streams.master_busy.update((k, ev) for k in keys)
            return
        with self._reduce_from():       # (behind the current stream and "wgrad2" as above, but "wgrad2" only where it exists)
            for k in keys:
                g = tr.model.bank.groups[k]["flat"]["g"]
                if k == "encoder_0" and self.head_inflight is not None:       # the tail slice is already in flight (see hook_head)
                    (off, h), self.head_inflight = self.head_inflight, None
                    self.handles.append(h)
                    self.marks.append((k + "[head]", (g.numel() - off) * 4))      # one mark per handle (dp_wait_ms)
                    g = g[:off]
                self.handles.append(D.allreduce_bucket(g, tr.world_size, tr.process_group))
                self.marks.append((k, g.numel() * 4))

    def finish(self, keys):
        """Wait for the buckets, one fused Adam launch per key that has not stepped early (TF semantics, Appendix A.12), the converted
        weight copies.  (HIP-graph mode: the python step counters advance outside.)"""
        tr, handles = self.tr, self.handles
        # data parallel: what the launching stream WAITS at the end of the backward pass, in its parts (JOIN_TIMING: the join alone)
        timed = self.graph_lr is None and not JOIN_TIMING and any(h is not None for h in handles) and not torch.cuda.is_current_stream_capturing()
        if timed:
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(handles) + 2)]
            evs[0].record()
        self.join("tail")
        if timed:
            evs[1].record()
            for i, h in enumerate(handles):
                if h is not None:
                    h.wait()
                evs[2 + i].record()
            self.dp_wait_events.append((evs, self.marks))
            handles = []
        D.wait_all(handles)
        tr._adam([k for k in keys if k not in self.stepped], self.graph_lr)     # (the list is complete before _adam adds to the set)
        self.begin(self.graph_lr)               # (handles, marks and the stepped keys: the step's optimizer work is complete)
        ops.Streams.master_busy.clear()         # (the join above ordered this stream behind every early Adam)
        ops.Streams.epoch += 1                  # lazy weight conversions of this step are ordered before everything that follows
        ops.weights_changed(tr.model.nets.prep, bump=self.graph_lr is None)       # (one batched refresh of the converted copies, the fp8 scales)

    def dp_wait_ms(self):
        """Data parallel: mean time per step the launching stream waited at the end of the backward pass -- for the weight-gradient
        streams to drain (`side_streams`), then, bucket by bucket in launch order, for each gradient all-reduce that had not
        finished by then (`<key>` with its bytes; 0 when the collective was fully hidden behind the backward pass).  Synchronises."""
        if not self.dp_wait_events:
            return None
        torch.cuda.synchronize(self.tr.device)
        out, n = {}, len(self.dp_wait_events)
        for evs, marks in self.dp_wait_events:       # (segment_done keeps one mark per handle: len(evs) == len(marks) + 2)
            for i, name in enumerate(["side_streams"] + ["{}:{}B".format(*m) for m in marks]):
                out[name] = out.get(name, 0.0) + evs[i].elapsed_time(evs[i + 1])
        return {k: round(v / n, 4) for k, v in out.items()}


class StepGraph(object):
    """``trainer.graph`` once graph mode is used (``Trainer._graph_step`` decides when to warm up, capture and replay): static input /
    noise buffers of one batch shape (``tps_u``: the TPS uniforms of a ``use_tps`` model), the device scalar ``lr`` for Adam's step size, the count of ``eager`` warm-up steps, and the
    capture -- ``graphs`` (empty until captured), the ``bounds`` between them, the schedule signature ``sig`` it baked in and
    ``img_src``, the captured step's buffers that the image logs are rendered from after a replay.
    Data parallel: the step is captured as a SEQUENCE of graphs, cut wherever the eager step talks to the other ranks (DESIGN
    section 7).  One python pass records all segments (the tape objects simply live on between them; the graphs share one memory
    pool and are always replayed in capture order); at replay the collectives run eagerly in between."""

    def __init__(self, trainer, B, S):
        self.tr, self.shape, dev = weakref.proxy(trainer), (B, S), trainer.device
        self.inputs = {k: torch.empty((B, S, S, 3), dtype=torch.float32, device=dev) for k in trainer.model.inputs}
        self.noise = {k: torch.empty_like(v) for k, v in trainer.draw_noise(B).items()}
        # `use_tps`: the uniforms of the in-graph TPS of both views.  NOT one of draw_noise's keys: the eager step draws them in
        # make_tps, before the window corner, and the generator's stream (checkpoints carry its state) stays that one
        self.tps_u = torch.empty((2 * B, TPS.N_UNIFORMS), dtype=torch.float32, device=dev) if trainer.model.use_tps else None
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sig, self.eager, self.graphs, self.bounds, self.img_src = None, 0, [], [], None
        self.capturing, self._pool, self._stream, self._cur = False, None, None, None       # capturing: inside capture()

    def capture(self, run_step, sig):
        """Record ``run_step()`` -- one whole step on the static buffers -- into ``graphs``; capturing does not execute."""
        dev = self.tr.device
        torch.cuda.synchronize(dev)
        keep = self.graphs, self.img_src        # (a re-capture: the previous graphs and their pool live until this one is complete)
        self.graphs, self.bounds, self.img_src = [], [], None
        self.capturing, self._pool, self._stream = True, torch.cuda.graph_pool_handle(), torch.cuda.Stream(dev)
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        try:
            with torch.cuda.stream(self._stream):
                self._segment_begin()
                run_step()
                self._segment_end()
        except BaseException:
            # leave the stream usable for the eager trainer: end the open capture (its graph is discarded), rejoin the side
            # streams, and stop trying to capture
            with contextlib.suppress(Exception), torch.cuda.stream(self._stream):
                if self._cur is not None:
                    ops.Streams.join(dev, names=("wgrad", "aux1", "aux2", "aux", "pre"))
                    self._cur.capture_end()
            self.tr._graph_enabled, self.tr.graph = False, None
            raise
        finally:
            self.capturing, self._cur = False, None
        torch.cuda.current_stream(dev).wait_stream(self._stream)
        torch.cuda.synchronize(dev)
        self.sig = sig

    def _segment_begin(self):
        self._cur = torch.cuda.CUDAGraph()
        self._cur.capture_begin(pool=self._pool)

    def _segment_end(self):
        ops.Streams.join(self.tr.device, names=("wgrad", "aux"))      # every forked stream rejoins before the capture ends
        self._cur.capture_end()
        self.graphs.append(self._cur)
        self._cur = None

    def boundary(self, kind, payload):
        """Called from inside the step while it is being captured: close the running segment, note what has to happen between
        it and the next one (kind "grads": all-reduce these keys' buckets; "scalars": average this tensor), open the next."""
        self._segment_end()
        self.bounds.append((kind, payload))
        self._segment_begin()

    def replay(self):
        tr, bank, handles = self.tr, self.tr.model.bank, []
        last_grads = max([i for i, (kind, _) in enumerate(self.bounds) if kind == "grads"], default=-1)
        for i, (graph, (kind, payload)) in enumerate(zip(self.graphs, self.bounds + [(None, None)])):
            graph.replay()
            if kind == "grads":
                handles += [D.allreduce_bucket(bank.groups[k]["flat"]["g"], tr.world_size, tr.process_group) for k in payload]
                if i == last_grads:
                    D.wait_all(handles)             # the next segment is the optimizer
            elif kind == "scalars":
                D.average_scalars(payload, tr.world_size, tr.process_group)
