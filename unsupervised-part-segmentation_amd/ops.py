"""Host-side operators over the C ABI: tap geometry for TF 'SAME' convolutions and the autograd
wrappers (forward / dgrad / wgrad) that let PyTorch own the tape while every FLOP runs in
libupsparts_hip.so.  Reference semantics: cub/code/nn.py (conv2d 617-711, residual_block 1042-1056,
upsample 834-847), SURVEY.md Appendix A.

Activations are NHWC tensors whose last dimension is the PHYSICAL channel count (multiple of 8);
weights stay fp32 in the TF variable layout HWIO and are re-laid-out / converted once per optimizer step.

fp16 forward tensors (``fmt = L.F16``, the mask decoder: 10 mantissa bits instead of bf16's 7 at the same MFMA rate -- what
north_star's part-mask IoU >= 0.99 needs, tests/bf16_emulation_study.py) live in torch.bfloat16 CONTAINERS: the autograd engine casts
every returned gradient to the dtype of the forward tensor, and the gradients of these layers are bf16 (range).  The format
travels beside the tensor (nets.Act.fmt, ConvFn's ``fmt`` argument); nothing but the HIP kernels reads those bits.
"""
import ctypes as C
import os

import torch

from . import lib as L
from . import switches as SW


def round8(c):
    return (c + 7) // 8 * 8


def same_geometry(size, k, stride):
    """TF 'SAME': out = ceil(in/stride); pad_before = pad_total // 2 (Appendix A.1)."""
    out = -(-size // stride)
    pad_total = max((out - 1) * stride + k - size, 0)
    return out, pad_total // 2


class _Workspace(object):
    """Grow-only device scratch, one buffer per (device, stream): launches on different HIP streams may overlap."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes, device):
        key = (device, L.raw_stream(device))
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


WORKSPACE = _Workspace()
COLSUM_WS = _Workspace()


class Streams(object):
    """Side HIP streams of the training step.  ``wgrad``: every layer's weight gradient is enqueued there while the
    input gradient continues on the launching stream (the two are independent; small layers that cannot fill 256 CUs
    then overlap).  ``aux``: the critics + the appearance code of the whole views, which the main path only needs
    again at the encoder_0 backward.  UPS_NO_OVERLAP=1 keeps everything on one stream (A/B runs, debugging)."""
    enabled = not SW.flag("UPS_NO_OVERLAP")
    _pool = {}
    _raw = {}       # (name, device index) -> raw hipStream_t
    epoch = 0          # bumped by the trainer at the end of every step (all side streams joined): scopes WeightCopy.ready
    master_busy = {}   # optimizer key -> event on the "wgrad" stream behind that key's early Adam launch (stepsync.GradSync: set in segment_done, cleared by finish / abort)
    _alive = {}     # device index -> tensors the "wgrad" stream still reads.  Holding references until the next join keeps
                    # their memory out of the allocator without record_stream (whose deferred frees made the caching
                    # allocator reserve ~9x the live set: 84 GB at B = 64); once the launching stream has waited for the
                    # side stream, dropping them is safe -- every later use of that memory is ordered behind the join.

    @classmethod
    def keep(cls, device, *tensors):
        cls._alive.setdefault(torch.device(device).index, []).extend(tensors)

    # Stream plan.  "full": every logical stream is a HIP stream of its own (seven with the launching stream) -- the fastest form on
    # ONE rank.  "compact": the logical streams fold onto three -- launching stream, "wgrad" (weight gradients
    # and their CoordConv rows), "aux" (target features, appearance code, the three critics) -- which leaves the fourth of the
    # four hardware queues (GPU_MAX_HW_QUEUES) to the collectives' stream under data parallelism: more than four ACTIVE queues are
    # time-sliced by the hardware scheduler (+30 % on the step).  The trainer picks the plan (`stream_plan`, model.Trainer).
    COMPACT_ALIAS = {"pre": "aux", "aux1": "aux", "aux2": "aux", "wgrad2": "wgrad"}
    alias = {}

    @classmethod
    def set_plan(cls, plan):
        if plan not in ("full", "compact"):
            raise ValueError("stream plan '{}' (full | compact)".format(plan))
        cls.alias = dict(cls.COMPACT_ALIAS) if plan == "compact" else {}

    @classmethod
    def get(cls, name, device):
        name = cls.alias.get(name, name)
        key = (name, torch.device(device).index)
        st = cls._pool.get(key)
        if st is None:
            st = torch.cuda.Stream(device=device)
            cls._pool[key] = st
            cls._raw[key] = st.cuda_stream
        return st

    @classmethod
    def wgrad_behind(cls, device, current=True, create=False):
        """Put the weight-gradient stream behind what a key's finished backward segment left in flight: the current stream
        (`current`; not from inside the backward pass, where the hook of a layer runs right after its weight gradient was enqueued)
        and then the CoordConv rows on "wgrad2".  `create`: make "wgrad2" if it does not exist yet -- the single-rank path does, the
        data-parallel paths must not (which streams share a hardware queue depends on the order they are created in,
        docs/design/negative_results.md).  Returns the "wgrad" stream."""
        side = cls.get("wgrad", device)
        if current:
            side.wait_stream(torch.cuda.current_stream(device))
        w2 = cls.get("wgrad2", device) if create else cls._pool.get(("wgrad2", torch.device(device).index))
        if w2 is not None:
            side.wait_stream(w2)
        return side

    _pads = []

    @classmethod
    def on_aux(cls, device):
        cur, idx = L.raw_stream(device), torch.device(device).index
        return any(cls._raw.get((n, idx)) == cur for n in ("aux", "aux1", "aux2"))      # (aux1 / aux2: critics two and three)

    @classmethod
    def join(cls, device, names=("wgrad", "aux")):
        """The current stream waits for everything enqueued on the side streams so far."""
        if not cls.enabled:
            return
        cur = torch.cuda.current_stream(device)
        if "wgrad" in names:
            names = tuple(names) + ("wgrad2",)          # the CoordConv rows of the weight gradients (conv_wgrad) belong to it
        if "aux" in names:
            names = tuple(names) + ("aux1", "aux2")         # critics two and three (Trainer._critics)
        seen = set()
        for n in names:
            n = cls.alias.get(n, n)
            if n in seen:
                continue
            seen.add(n)
            st = cls._pool.get((n, torch.device(device).index))
            if st is not None and st != cur:
                cur.wait_stream(st)
        if "wgrad" in names:
            cls._alive.pop(torch.device(device).index, None)


class KernelTimer(object):
    """bench.py hook: HIP events (recorded on the launch stream) around every launch of the patch kernel for one named
    convolution -- its forward and its input-gradient launches: the same kernel on the same problem size -- so the roofline
    figure is that kernel's own duration, measured live."""
    layer, enabled, events, flops = None, False, [], 0.0
    kinds = []        # "fwd" / "dgrad" per timed launch

    @classmethod
    def active(cls):
        # (events recorded while a HIP graph is being captured become graph nodes and cannot be read back: replayed steps are not timed)
        return cls.enabled and not torch.cuda.is_current_stream_capturing()

    @classmethod
    def mean_ms(cls, kind=None):
        ev = [e for e, k in zip(cls.events, cls.kinds) if kind is None or k == kind]
        return sum(a.elapsed_time(b) for a, b in ev) / max(1, len(ev))


class WeightVersion(object):
    """Bumped whenever fp32 master weights change (weights_changed); every WeightCopy compares its own version with it."""
    value = 0


class SignBits(object):
    """Bit-packed activation signs (ups_conv_desc.sign_out / dact_bits, round 5).  The input gradient of a convolution needs one
    bit of every element of the layer's forward input -- the sign, for act' -- and re-read the whole 16-bit tensor for it.  The
    PRODUCER of such a tensor (a convolution's epilogue, the x2 bilinear kernel) now also writes [n,h,w,c/8] sign bytes, the handle
    carries them (nets.Act.bits) and the consuming convolution's backward passes them to ups_conv_igemm next to `dact`.
    The caller that will keep the bits asks for them with ``Handoff.want_bits`` and finds them in ``Handoff.bits`` after the call."""
    stats = None        # a dict when a probe wants to know which input gradients ran without bits (tools/probes/sign_bits_coverage.py)


class Handoff(object):
    """What ONE producer call (ops.conv, BilinearFn, MaxPoolFn: their last argument ``side``) is given and gives back beside its
    tensor; made by the caller for that call, never kept by the operator or its autograd context (the nets.Act carries the results).
    In: ``f8_in`` -- the fp8 copy of the input its producer wrote (Fp8.handle) or None; ``f8_out_act`` -- the activation-on-load of
    the output's consumer, None: no fp8 copy of the output is wanted (ops.conv; the point-wise producers take it as `act` and
    write whenever their site does); ``want_bits`` -- the output's sign bytes (SignBits) are wanted.
    Out, None where the call wrote nothing: ``f8_out`` -- the output's fp8 copy (Fp8.handle); ``bits`` -- its sign bytes."""
    __slots__ = ("f8_in", "f8_out_act", "want_bits", "f8_out", "bits", "__weakref__")

    def __init__(self, f8_in=None, f8_out_act=None, want_bits=False):
        self.f8_in, self.f8_out_act, self.want_bits = f8_in, f8_out_act, want_bits
        self.f8_out = self.bits = None


class WeightCopy(object):
    """One converted copy of a layer's fp32 master weights (blocked-K 16-bit / fp32, depth-to-space, e4m3 forward / input-gradient,
    deconvolution operands).  ``bufs``: name -> device buffer, allocated once (the pointers sit in the batched refresh's item tables
    and in captured graphs) -- what the operators read.  ``convert()`` enqueues the launches that fill them on the current stream.
    ``item`` = (dtype_code, hi, wi) where ups_weight_prep_batch can make the copy, else None.  A copy of a trainable layer that
    has a registry is re-made by PrepRegistry.refresh after every optimizer step; all others convert in ``get()`` once
    WeightVersion has moved -- a frozen layer's only the first time and after ``invalidate()``."""
    __slots__ = ("layer", "bufs", "convert", "item", "version", "ready")

    def __init__(self, layer, bufs, convert, item=None):
        self.layer, self.bufs, self.convert, self.item = layer, bufs, convert, item
        self.version = -1
        self.ready = None       # (raw stream, event, streams that have waited for it, Streams.epoch) behind a lazy conversion
        if layer.registry is not None and not layer.frozen:
            layer.registry.register(self)

    def invalidate(self):
        self.version = -1

    def get(self):
        """``bufs``, holding the current weights as far as the current stream is concerned."""
        if self.version != WeightVersion.value and not (self.version >= 0 and self.layer.frozen):
            self._wait_master()
            self.convert()
            self.version = WeightVersion.value
            # A lazy conversion was just enqueued on the current stream: remember where, so that a consumer on ANOTHER stream of the
            # same step (the appearance encoder first runs on "aux", the frozen trunk on "pre", both again on the launching stream)
            # waits for it instead of racing with it.  The refresh at the end of a step runs on the launching stream, from which
            # every side stream forks afterwards: it clears the mark.
            dev = self.layer.V.device
            if torch.cuda.is_current_stream_capturing():       # (captures start after eager steps: nothing converts lazily in them)
                self.ready = None
            else:
                self.ready = (L.raw_stream(dev), torch.cuda.current_stream(dev).record_event(), set(), Streams.epoch)
        elif self.ready is not None:
            self._wait_ready()
        return self.bufs

    def _wait_ready(self):
        rd = self.ready
        if rd[3] != Streams.epoch:          # an earlier step's conversion: every stream has been joined and re-forked since
            self.ready = None
            return
        dev = self.layer.V.device
        cur = L.raw_stream(dev)
        if cur != rd[0] and cur not in rd[2] and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(dev).wait_event(rd[1])
            rd[2].add(cur)

    def _wait_master(self):
        """Before reading the fp32 master weights on this stream: wait for an Adam launch of this layer's optimizer key that is
        still in flight on the weight-gradient stream (the trainer's early per-key Adam; keys match by substring, as edflow's
        variable lists do)."""
        if Streams.master_busy:
            cur = torch.cuda.current_stream(self.layer.V.device)
            for key, ev in Streams.master_busy.items():
                if key in self.layer.name:
                    cur.wait_event(ev)


class PrepRegistry(object):
    """The WeightCopy objects of a model's trainable layers.  ``refresh`` re-makes all of them after the optimizer step: the
    blocked-K copies (those with an ``item``) by ONE ups_weight_prep_batch launch per dtype instead of two small launches per layer
    and step, the others (depth-to-space, e4m3, deconvolution operands) by their own ``convert()``.  The device-side item tables
    are built at the first refresh after a registration."""

    def __init__(self):
        self.copies = []
        self.tables = {}           # dtype_code -> (items_dev, prefix_dev, n, total_blocks)
        self.dirty = True

    def register(self, copy):
        self.copies.append(copy)
        self.dirty = self.dirty or copy.item is not None

    def _build(self):
        self.tables = {}
        lib = L.load()
        batched = [c for c in self.copies if c.item is not None]
        for dcode in sorted(set(c.item[0] for c in batched)):
            ents = [c for c in batched if c.item[0] == dcode]
            arr = (L.PrepItem * len(ents))()
            prefix = [0]
            for i, c in enumerate(ents):
                lay, ent, (_, hi, wi), it = c.layer, c.bufs, c.item, arr[i]
                it.src = lay.V.data_ptr()
                it.w_fwd = ent["w_fwd"].data_ptr() if ent["w_fwd"] is not None else None
                it.w_dgrad = ent["w_dgrad"].data_ptr() if ent["w_dgrad"] is not None else None
                it.ctab = ent["ctab"].data_ptr() if ent["ctab"] is not None else None
                it.ntaps, it.cin_v, it.ci_log, it.co = lay.k * lay.k, lay.cin_v, lay.ci_log, lay.co
                it.ci_pad, it.dgrad_rows, it.dgrad_k = round8(lay.ci_log), lay.ci_log, round8(lay.co)
                it.kh = it.kw = lay.k
                it.in_sy = it.in_sx = lay.stride
                dy, dx, _ = lay.fwd_taps(hi, wi)
                for r in range(3):
                    it.dy[r] = dy[r * lay.k] if r < lay.k else 0
                    it.dx[r] = dx[r] if r < lay.k else 0
                it.ax, it.ay = 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)
                prefix.append(prefix[-1] + lib.ups_prep_item_blocks(C.byref(it), dcode))
            dev = ents[0].layer.V.device
            items_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            prefix_dev = torch.tensor(prefix, dtype=torch.int64, device=dev)
            self.tables[dcode] = (items_dev, prefix_dev, len(ents), prefix[-1])
        self.dirty = False

    def refresh(self):
        """Re-convert every registered copy from the current fp32 master weights, on the current stream (the caller has ordered it
        behind every optimizer launch and forks the side streams from it afterwards: no ready mark is needed)."""
        if self.dirty:
            self._build()
        for dcode, (items_dev, prefix_dev, n, total) in self.tables.items():
            L.call("ups_weight_prep_batch", L.ptr(items_dev), L.ptr(prefix_dev), n, total, dcode, L.stream())
        for c in self.copies:
            if c.item is None:
                c.convert()
            c.version = WeightVersion.value
            c.ready = None


def weights_changed(registry=None, bump=True):
    """The fp32 master weights have changed (optimizer step, initialisation, restore).  bump=False: a step inside a HIP graph -- the
    graph's own launches re-make the copies at every replay, the host-side counter stays.  With the model's registry its copies are
    re-made here and fp8 mode's delayed scales take their step; every other copy converts at its next use."""
    if bump:
        WeightVersion.value += 1
    if registry is not None:
        registry.refresh()
        if Fp8.enabled:
            Fp8.after_step()


class Fp8State(object):
    """fp8 forward of the wide 3x3 / stride-1 convolutions (BASELINE config #5: e4m3 MFMA operands, fp32 accumulate, bf16
    tensors; ``precision: fp8`` in the config).  Weights are scaled per output channel when they are converted; activations
    use delayed per-tensor scaling: every launch records max |act(x)| (kernel epilogue, 64 atomic slots per layer) and
    ``update()`` -- once per step, three tiny launches for all layers -- turns it into the next step's scale
    448 * MARGIN / amax.  A layer's first launch scales from the tensor at hand.

    One instance per model (``TrainModel.fp8``): scale slots, hand-off state, switches and counters.  The operators
    reach the state of the model that is running through the module-level ``Fp8`` proxy; ``TrainModel`` / ``Trainer`` activate
    their own instance before they touch a layer, so two models alive in one process (a trainer plus an evaluation model, a
    test sweep) never share slots.  Layers keep the slot numbers of THEIR model's state in ``layer.f8`` (scale slots, ``primed``
    flags, producer sites; ``generation`` guards against a layer being driven under a foreign state).  The e4m3 weight copies are
    WeightCopy objects like every other converted copy: the model's PrepRegistry re-makes them after the optimizer step."""
    MARGIN = 0.5            # headroom for the step-to-step growth of amax (e4m3 max normal = 448)
    MAX_LAYERS = 512
    E5M2_MAX = 57344.0
    _generations = 0

    def __init__(self, enabled=False, copy_only=None):
        Fp8State._generations += 1
        self.generation = Fp8State._generations
        self.enabled = bool(enabled)
        self.amax = None            # [MAX_LAYERS, 64] fp32
        self.scale = None           # [MAX_LAYERS] fp32
        self.fmax = None            # [MAX_LAYERS] fp32: largest normal of the slot's format
        self.count = 0
        self.GRAD = True            # input gradients of the fp8 layers on e5m2 operands (False: bf16 kernels)
        # (weight gradients of the wide 3x3 layers: on e4m3 x e5m2 operands, conv_wgrad3x3_f8.hip, wherever the gradient arrives with
        # its producer's e5m2 copy -- eligible_wgrad)
        # COPY_ONLY: a layer takes the fp8 kernels only when its operand arrives quantised (a copy written by the producing
        # bilinear / convolution kernel); layers whose operand would have to be converted inside the kernel (24 staging
        # registers, one block per CU: slower than bf16) stay on the bf16 kernels.  None: follows PRODUCER.
        # (config key `fp8_copy_only`)
        self.COPY_ONLY = copy_only
        # fp8 copies handed from layer to layer: the producing convolution's epilogue writes e4m3(act(out) * scale) next to its
        # bf16 output (scale = the delayed scale of that tensor), the consuming convolution stages those bytes without any
        # conversion.  nets.Scope passes the handle ({"t": uint8 tensor, "act": UPS_ACT_*, "slot": scale slot, "site"}) along as
        # arguments of the calls: Handoff.f8_in into ops.conv, Handoff.f8_out out of it; no state here outlives a call.
        # UPS_F8_PRODUCER=0 switches the hand-off off (every eligible layer then converts its bf16 operand inside the kernel).
        self.PRODUCER = SW.flag("UPS_F8_PRODUCER")
        self.skip_nonfinite = False # the trainer's `skip_nonfinite` key: update() keeps the scale of a slot whose maximum is not finite
        self.steps = 0              # update() calls so far (a tensor's copy starts one step after its first maximum was recorded)
        self.stats = {"fwd_f8": 0, "fwd_copy_in": 0, "fwd_copy_out": 0, "dgrad_f8": 0, "dgrad_copy_in": 0, "dgrad_copy_out": 0,
                      "wgrad_f8": 0}
        self.grad_side = {}         # data_ptr of a gradient tensor -> (weakref to it, its e5m2 copy): dgrad epilogue -> next dgrad

    def slot(self, device):
        if self.amax is None or self.amax.device != device:
            self.amax = torch.zeros((self.MAX_LAYERS, 64), dtype=torch.float32, device=device)
            self.scale = torch.ones((self.MAX_LAYERS,), dtype=torch.float32, device=device)
            self.fmax = torch.full((self.MAX_LAYERS,), 448.0, dtype=torch.float32, device=device)   # e4m3; gradient slots: e5m2
            self.count = 0
        i = self.count
        self.count += 1
        if i >= self.MAX_LAYERS:
            raise L.UpsError("more than {} fp8 layers".format(self.MAX_LAYERS))
        return i

    def update(self):
        """Next step's activation scales from this step's maxima (layers that did not run keep theirs)."""
        if self.amax is None or self.count == 0:
            return
        n = self.count
        m = self.amax[:n].amax(dim=1)
        ok = m > 0
        if self.skip_nonfinite:     # (`skip_nonfinite`: a slot whose recorded maximum is inf or NaN keeps its scale instead of taking 0 / NaN)
            ok = ok & torch.isfinite(m)
        self.scale[:n] = torch.where(ok, (self.fmax[:n] * self.MARGIN) / m.clamp_min(1e-30), self.scale[:n])
        self.amax[:n].zero_()
        self.steps += 1

    def after_step(self):
        """After the optimizer step: new activation scales (the e4m3 weight copies are PrepRegistry.refresh's)."""
        self.update()
        self.grad_side.clear()          # copies nobody read this step are released (they pinned a gradient-sized tensor each)

    @staticmethod
    def wanted(site):
        """A producer keeps writing its copy only while somebody reads it: after two unread copies the site goes quiet."""
        return not (site.get("emitted", 0) >= 2 and site.get("used", 0) == 0)

    def site(self, holder, key, device, e5m2=False, layer=None):
        """The producer site stored at holder[key] (made on first use: its scale slot and the step it was born in), or None once
        the site has gone quiet (``wanted``).  e5m2: the copy is a gradient's, its slot takes that format's range.  layer: the
        holder is that layer's ``f8`` -- the site then records this state's generation and is read back through ``layer_entry``.
        Open: the point-wise sites (BilinearFn, MaxPoolFn: holder = a dict owned by the Scope) carry no generation guard."""
        so = holder.get(key) if layer is None else self.layer_entry(layer, key)
        if so is None:
            so = holder[key] = {"slot": self.slot(device), "born": self.steps}
            if layer is not None:
                so["gen"] = self.generation
            if e5m2:
                self.fmax[so["slot"]] = self.E5M2_MAX
        return so if self.wanted(so) else None

    def emit(self, site, shape, device):
        """The uint8 tensor this launch writes the site's copy into, or None in the step the site was born in (the launch then only
        records the maximum: the delayed scale of the tensor exists one ``update()`` later)."""
        if self.steps <= site["born"]:
            return None
        site["emitted"] = site.get("emitted", 0) + 1
        return torch.empty(shape, dtype=torch.uint8, device=device)

    @staticmethod
    def handle(site, t, act=None):
        """What a producer hands on: ``Handoff.f8_out``, the next call's ``Handoff.f8_in`` (act = the activation the copy was
        quantised behind) or, without `act`, the argument of ``register_grad_copy``."""
        h = {"t": t, "slot": site["slot"], "site": site}
        if act is not None:
            h["act"] = act
        return h

    @staticmethod
    def mark_used(copy):
        site = copy.get("site")
        if site is not None:
            site["used"] = site.get("used", 0) + 1

    def copy_only(self):
        return self.PRODUCER if self.COPY_ONLY is None else self.COPY_ONLY

    @staticmethod
    def usable(src, layer, x, ldi):
        """src (a producer's fp8 copy handle or None) is this layer's input, quantised with this layer's activation-on-load."""
        return (src is not None and src.get("t") is not None and src["act"] == layer.act_in and tuple(src["t"].shape) == tuple(x.shape)
                and layer.co > 32 and ldi % 16 == 0)

    def register_grad_copy(self, t, copy):
        import weakref
        if len(self.grad_side) > 256:
            self.grad_side.clear()
        # t._version: the autograd engine's InputBuffer accumulates other branches INTO a buffered gradient in place when it
        # holds the last reference (a weakref does not count as one) -- the same object then arrives holding g1 + g2 while the
        # copy still holds quantised g1; every in-place add bumps the version counter
        self.grad_side[t.data_ptr()] = (weakref.ref(t), tuple(t.shape), copy, t._version)

    def grad_copy(self, g):
        """The e5m2 copy of exactly this tensor object, unmodified since the copy was written, or None."""
        ent = self.grad_side.pop(g.data_ptr(), None)
        if ent is None or ent[0]() is not g or ent[1] != tuple(g.shape) or ent[3] != g._version:
            return None
        return ent[2]

    def layer_entry(self, layer, key):
        """A layer's fp8 entry (``layer.f8``: scale slot, primed flag or producer site) -- only if it was made under THIS state."""
        ent = layer.f8.get(key)
        if ent is not None and ent.get("gen") != self.generation:
            raise L.UpsError("{}: fp8 entry '{}' belongs to another model's Fp8State (generation {} != {}): a layer is being "
                             "driven while a different model's state is active".format(layer.name, key, ent.get("gen"), self.generation))
        return ent

    def eligible_grad(self, layer, g, x):
        """Input gradient of a stride-1 3x3 layer on fp8 operands: K = output channels of the forward."""
        return (self.enabled and self.GRAD and g.dtype == torch.bfloat16 and layer.k == 3 and layer.stride == 1
                and x.shape[1] % 16 == 0 and x.shape[2] % 16 == 0 and round8(layer.co) % 64 == 0 and layer.ci_log >= 64
                and g.shape[-1] >= round8(layer.co))

    def eligible_wgrad(self, layer, g, x, mask):
        """Weight gradient on the block-scaled fp8 MFMA (mirrors eligible8 of conv_wgrad3x3_f8.hip): K = pixels."""
        return (self.enabled and mask is None and g.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
                and layer.k == 3 and layer.stride == 1 and x.shape[1] % 16 == 0 and x.shape[2] % 16 == 0
                and round8(layer.ci_log) % 64 == 0 and layer.co % 128 == 0 and g.shape[-1] % 16 == 0)

    def eligible(self, layer, x):
        return (self.enabled and x.dtype == torch.bfloat16 and layer.k == 3 and layer.stride == 1
                and x.shape[1] % 16 == 0 and x.shape[2] % 16 == 0 and round8(layer.ci_log) % 64 == 0 and layer.co >= 64)


class _Fp8Proxy(object):
    """``ops.Fp8``: attribute access goes to the ACTIVE Fp8State (the running model's; a disabled default otherwise)."""

    def __init__(self):
        object.__setattr__(self, "_cur", Fp8State(False))

    def activate(self, state):
        object.__setattr__(self, "_cur", state)
        return state

    @property
    def current(self):
        return object.__getattribute__(self, "_cur")

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_cur"), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_cur"), name, value)


Fp8 = _Fp8Proxy()


class fp8_scope(object):
    """``with ops.fp8_scope(enabled=True, copy_only=False) as F:`` -- a fresh Fp8State active inside the block (kernel-level tests,
    tools), the previous one restored afterwards."""

    def __init__(self, enabled=True, copy_only=None):
        self.state = Fp8State(enabled, copy_only)

    def __enter__(self):
        self.prev = Fp8.current
        return Fp8.activate(self.state)

    def __exit__(self, *a):
        Fp8.activate(self.prev)


class _Layer(object):
    """What ConvLayer and DeconvLayer share: the master weights V and their converted copies (``copies``: key -> WeightCopy)."""

    def __init__(self, name, V):
        self.name, self.V = name, V
        self.frozen = False         # frozen weights (perceptual trunk): converted copies survive optimizer steps
        self.after_wgrad = None     # optional callback run right after this layer's weight gradient has been enqueued
        self.registry = None        # PrepRegistry of the owning model (refresh after the optimizer) or None (lazy per-layer prep)
        self.f16 = False            # forward tensors of this layer are fp16 (nets.Scope.fmt)
        self.copies = {}

    def invalidate(self):
        """The master weights were overwritten behind WeightVersion's back (a frozen layer's, on load): convert again at next use."""
        for c in self.copies.values():
            c.invalidate()


class ConvLayer(_Layer):
    """One conv2d variable pair (V [kh,kw,Cin(+2),Cout] HWIO fp32, b [Cout]) + its launch geometry."""

    def __init__(self, name, V, b, k, stride, coords, act_in, slope=0.2):
        _Layer.__init__(self, name, V)
        self.b = b
        self.k, self.stride, self.coords = k, stride, coords
        self.act_in = L.ACT[act_in] if not isinstance(act_in, int) else act_in
        self.slope = slope
        self.cin_v = V.shape[2]
        self.ci_log = self.cin_v - (2 if coords else 0)
        self.co = V.shape[3]
        self.grad_V = None          # optional preallocated views into a flat gradient buffer
        self.grad_b = None
        # post-activation storage (ups_conv_desc.out_act / res_act): in_post = the input tensor already holds act_in(x) -- the
        # forward and the weight gradient stage it as it is (LDS-DMA patch), the input gradient still reads act' off its sign;
        # out_act = the output is stored as out_act(y) because its consumer would apply that activation on load
        self.in_post = False
        self.out_act = L.ACT_NONE
        self.f8 = {}                # fp8 mode, per Fp8State.layer_entry: scale slots + primed flags ("f8", "f8g", "f8w"), producer sites

    # ---- converted weights (WeightCopy: re-made when the optimizer has stepped)
    def prepared(self, dtype_code, hi, wi):
        """Blocked-K weights [tap][k-chunk][row][64 B] of the forward ("w_fwd") and the input gradient ("w_dgrad") + "ctab"."""
        key = (dtype_code, hi, wi)
        copy = self.copies.get(key)
        if copy is None:
            dev, td = self.V.device, L.torch_dtype(dtype_code)
            ntaps, ci_pad = self.k * self.k, round8(self.ci_log)
            bk = 16 if dtype_code == L.F32 else 32
            # a layer with fp16 forward tensors: forward weights as fp16, input-gradient weights as bf16 (one copy each)
            want_f = not (self.f16 and dtype_code == L.BF16)
            want_d = dtype_code != L.F16
            ent = {"w_fwd": torch.empty((ntaps, -(-ci_pad // bk), self.co, bk), dtype=td, device=dev) if want_f else None,
                   "w_dgrad": torch.empty((ntaps, -(-round8(self.co) // bk), self.ci_log, bk), dtype=td, device=dev) if want_d else None,
                   "ctab": torch.empty((64, 3, self.co), dtype=torch.float32, device=dev) if (self.coords and want_f) else None}

            def convert():
                L.call("ups_weight_prep", L.ptr(self.V), ntaps, self.cin_v, self.ci_log, self.co, dtype_code,
                       L.ptr(ent["w_fwd"]), ci_pad, L.ptr(ent["w_dgrad"]), self.ci_log, round8(self.co), L.stream())
                if ent["ctab"] is not None:
                    dy, dx, _ = self.fwd_taps(hi, wi)
                    ax, ay = 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)     # nn.py:2145-2148 (xx / (H-1), yy / (W-1))
                    L.call("ups_coord_table", L.ptr(self.V), self.k, self.k, self.ci_log, self.co,
                           (C.c_int32 * 9)(*dy), (C.c_int32 * 9)(*dx), self.stride, self.stride, ax, ay,
                           L.ptr(ent["ctab"]), L.stream())
            copy = self.copies[key] = WeightCopy(self, ent, convert, item=key)
        return copy.get()

    def d2s_channels(self, x):
        """C of the depth-to-space input gradient (ups_conv_desc.d2s) when this layer / tensor can take it, else 0."""
        c = self.ci_log
        ok = (self.k == 3 and self.stride == 2 and x.dtype == torch.bfloat16 and c >= 8 and (c & (c - 1)) == 0
              and x.shape[-1] == c and x.shape[1] % 32 == 0 and x.shape[2] % 32 == 0)
        return c if ok else 0

    def prepared_d2s(self, hi, wi):
        """Weights ("w") of the one-launch input gradient of a 3x3 / stride-2 layer (ups_weight_prep_d2s); they depend on the input
        size through its 'SAME' pads alone."""
        _, pby = same_geometry(hi, 3, 2)
        _, pbx = same_geometry(wi, 3, 2)
        key = ("d2s", pby, pbx)
        copy = self.copies.get(key)
        if copy is None:
            w = torch.empty((9, -(-self.co // 32), 4 * self.ci_log, 32), dtype=torch.bfloat16, device=self.V.device)
            copy = self.copies[key] = WeightCopy(self, {"w": w}, lambda: L.call(
                "ups_weight_prep_d2s", L.ptr(self.V), self.cin_v, self.ci_log, self.co, pby, pbx, self.ci_log, L.ptr(w), L.stream()))
        return copy.get()

    def _prepared_e4m3(self, key, grad, rows, k, t):
        """An e4m3 weight copy for a GEMM of `rows` output rows over K = `k` ("w", scaled per row; "deq": the rows' dequantisation
        factors) + "slot": the delayed-scale slot of the tensor `t` it meets (grad: an e5m2 gradient, and the weights transposed),
        primed from `t` at the first launch that brings one."""
        st = Fp8.layer_entry(self, key)
        fmax = Fp8.E5M2_MAX if grad else 448.0
        if st is None:
            dev = self.V.device
            st = self.f8[key] = {"slot": Fp8.slot(dev), "primed": False, "gen": Fp8.generation}
            if grad:
                Fp8.fmax[st["slot"]] = fmax
            w = torch.empty((self.k * self.k, -(-k // 64), rows, 64), dtype=torch.uint8, device=dev)
            deq = torch.empty((rows,), dtype=torch.float32, device=dev)
            self.copies[key] = WeightCopy(self, {"w": w, "deq": deq, "slot": st["slot"]}, lambda: L.call(
                "ups_weight_prep_f8", L.ptr(self.V), self.k * self.k, self.cin_v, self.ci_log, self.co, int(grad),
                L.ptr(w), L.ptr(deq), L.stream()))
        ent = self.copies[key].get()
        if not st["primed"] and t is not None:
            m = t[..., :k].abs().amax().float()
            Fp8.scale[st["slot"]] = torch.where(m > 0, (fmax * Fp8.MARGIN) / m.clamp_min(1e-30), torch.ones_like(m))
            st["primed"] = True
        return ent

    def prepared_f8_grad(self, g):
        """e4m3 weights of the input-gradient GEMM (rows = input channels, scaled per row) + the gradient tensor's e5m2 scale slot."""
        return self._prepared_e4m3("f8g", True, self.ci_log, self.co, g)

    def prepared_f8_wgrad(self, x, fmt):
        """Scale slot of the forward input as the fp8 weight gradient quantises it (delayed scaling: the kernel records
        max |act(x)|, ops.Fp8.update turns it into the next step's scale; the first launch scales from the tensor at hand)."""
        ent = Fp8.layer_entry(self, "f8w")
        if ent is None:
            ent = self.f8["f8w"] = {"slot": Fp8.slot(self.V.device), "primed": False, "gen": Fp8.generation}
        if not ent["primed"]:
            xv = x.view(torch.float16) if fmt == L.F16 else x       # (fp16 forward tensors live in bf16 containers)
            m = xv[..., :round8(self.ci_log)].abs().amax().float()
            Fp8.scale[ent["slot"]] = torch.where(m > 0, (448.0 * Fp8.MARGIN) / m.clamp_min(1e-30), torch.ones_like(m))
            ent["primed"] = True
        return ent

    def prepared_f8(self, x):
        """e4m3 weights + per-channel dequantisation factors + this layer's activation-scale slot (the first launch of the layer
        scales from the tensor at hand: |act(x)| <= |x|)."""
        return self._prepared_e4m3("f8", False, self.co, self.ci_log, x)

    def out_hw(self, hi, wi):
        return same_geometry(hi, self.k, self.stride)[0], same_geometry(wi, self.k, self.stride)[0]

    def fwd_taps(self, hi, wi):
        _, pby = same_geometry(hi, self.k, self.stride)
        _, pbx = same_geometry(wi, self.k, self.stride)
        dy, dx, tw = [0] * 9, [0] * 9, [0] * 9
        for r in range(self.k):
            for s in range(self.k):
                t = r * self.k + s
                dy[t], dx[t], tw[t] = r - pby, s - pbx, t
        return dy, dx, tw


def _fill_taps(desc, dy, dx, tw, ntaps):
    for t in range(9):
        desc.tap_dy[t] = dy[t] if t < ntaps else 0
        desc.tap_dx[t] = dx[t] if t < ntaps else 0
        desc.tap_w[t] = tw[t] if t < ntaps else 0
    desc.ntaps = ntaps


SPLITK_WS_BYTES = 48 << 20


def _attach_ws(d, device):
    """Scratch of the split-K path of ups_conv_igemm (per stream; grown once to SPLITK_WS_BYTES)."""
    ws = WORKSPACE.get(SPLITK_WS_BYTES, device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()


def _conv_desc(dcode, src, in_dims, w, out, out_dims, taps, kh, kw, slope, in_stride=1, lattice=None):
    """The fields every ups_conv_desc shares; all others start at zero / NULL.  in_dims = (n, hi, wi, ci, ldi) of `src`;
    out_dims = (ho, wo, co, co_fill, ldo): the ho x wo results of the kh x kw taps = (dy, dx, weight index) land in `out` densely
    or, with lattice = (out_h, out_w, stride, oy, ox), on every stride-th pixel from (oy, ox) of an out_h x out_w tensor."""
    d = L.ConvDesc()
    d.dtype = dcode
    d.n, d.hi, d.wi, d.ci, d.ldi = in_dims
    d.ho, d.wo, d.co, d.co_fill, d.ldo = out_dims
    out_h, out_w, st, oy, ox = lattice if lattice is not None else (d.ho, d.wo, 1, 0, 0)
    d.out_h, d.out_w, d.out_sy, d.out_sx, d.out_oy, d.out_ox = out_h, out_w, st, st, oy, ox
    d.in_sy = d.in_sx = in_stride
    _fill_taps(d, taps[0], taps[1], taps[2], kh * kw)
    d.kh, d.kw = kh, kw
    d.act_slope = slope
    d.in_, d.w, d.out = src.data_ptr(), w.data_ptr(), out.data_ptr() if out is not None else None
    _attach_ws(d, src.device)
    return d


def _attach_dgrad(d, layer, x, x_bits, res):
    """Epilogue of an input-gradient launch: gx = act'(x) * (what the taps summed) (+ res); act' off x or off its sign bytes."""
    d.dact_kind = layer.act_in
    d.ldd = x.shape[-1]
    if layer.act_in != L.ACT_NONE:
        d.dact = x.data_ptr()
        d.dact_bits = x_bits.data_ptr() if x_bits is not None else None
    if res is not None:
        d.res, d.ldr = res.data_ptr(), res.shape[-1]


def _attach_f8_operand(d, prepare, t, src, stat):
    """The fp8 kernel's operands.  src (a producer's copy of the input tensor `t`, or None): its bytes and the scale they were
    written with; without one the kernel quantises `t` with this layer's delayed scale and records the maximum.  prepare:
    layer.prepared_f8 (stat "fwd") / layer.prepared_f8_grad ("dgrad"): the e4m3 weights and their dequantisation factors."""
    if src is not None:
        f8 = prepare(None)
        Fp8.stats[stat + "_copy_in"] += 1
        Fp8.mark_used(src)
        d.in_f8 = src["t"].data_ptr()
        d.f8_scale = Fp8.scale[src["slot"]:].data_ptr()
    else:
        f8 = prepare(t)
        d.f8_scale = Fp8.scale[f8["slot"]:].data_ptr()
        d.f8_amax = Fp8.amax[f8["slot"]].data_ptr()
    d.w = f8["w"].data_ptr()
    d.f8_deq = f8["deq"].data_ptr()
    Fp8.stats[stat + "_f8"] += 1


def _attach_f8_copy(d, site, shape, device, stat):
    """The epilogue records the output's maximum in the site's slot and, once its delayed scale exists, writes the fp8 copy:
    returns that tensor or None."""
    d.out_f8_amax = Fp8.amax[site["slot"]].data_ptr()
    t8 = Fp8.emit(site, shape, device)
    if t8 is not None:
        d.out_f8, d.out_f8_scale = t8.data_ptr(), Fp8.scale[site["slot"]:].data_ptr()
        Fp8.stats[stat] += 1
    return t8


def _launch_conv(d, layer, kind=None, flops=None):
    """ups_conv_igemm on the current stream.  kind ("fwd" / "dgrad"): a launch bench.py's roofline times when it watches this layer."""
    if kind is not None and KernelTimer.layer == layer.name and KernelTimer.active():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.call("ups_conv_igemm", C.byref(d), L.stream())
        e1.record()
        KernelTimer.events.append((e0, e1))
        KernelTimer.kinds.append(kind)
        if flops is not None:
            KernelTimer.flops = flops
    else:
        L.call("ups_conv_igemm", C.byref(d), L.stream())


def conv_forward(x, layer, res=None, out_f32=False, ldo=None, co_fill=None, mask=None, fmt=None, res_post=False, side=None):
    """out = conv(act(x) (+coords), V) + b (+ res);  x [n,hi,wi,ldi].  side: this call's Handoff (None: nothing in, nothing wanted).
    fmt = L.F16: x, res and (unless out_f32) out hold fp16 in bf16 containers (module docstring).
    mask = (hard_bits [B,hi,wi] int32, P): x is the UNMASKED view [B,hi,wi,ldi] and the convolution runs on the P*B part images
    x[b] * hard[b,:,:,p] (part-major) without materialising them (model.py:176-187, nn.py:81-113)."""
    n, hi, wi, ldi = x.shape
    if mask is not None:
        n = n * mask[1]
    dcode = L.dt(x) if fmt is None else fmt
    assert dcode != L.F16 or (x.dtype == torch.bfloat16 and mask is None and layer.f16)
    ho, wo = layer.out_hw(hi, wi)
    ent = layer.prepared(dcode, hi, wi)
    ldo = ldo if ldo is not None else (layer.co if out_f32 else round8(layer.co))
    co_fill = co_fill if co_fill is not None else ldo
    out = torch.empty((n, ho, wo, ldo), dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    d = _conv_desc(dcode, x, (n, hi, wi, round8(layer.ci_log), ldi), ent["w_fwd"], out, (ho, wo, layer.co, co_fill, ldo),
                   layer.fwd_taps(hi, wi), layer.k, layer.k, layer.slope, in_stride=layer.stride)
    d.act_in, d.out_f32 = (L.ACT_NONE if layer.in_post else layer.act_in), int(out_f32)
    d.out_act = layer.out_act
    d.bias = layer.b.data_ptr()
    d.coord_tab = ent["ctab"].data_ptr() if layer.coords else None
    if res is not None:
        d.res, d.ldr = res.data_ptr(), res.shape[-1]
        d.res_act = layer.act_in if res_post else L.ACT_NONE       # residual stored as act(x): inverted in the epilogue
        assert not (d.res_act and layer.act_in != L.ACT_LRELU), "only a leaky-ReLU residual can be stored post-activation"
    side = side if side is not None else Handoff()
    src, want_act = side.f8_in, side.f8_out_act
    if mask is not None:
        d.mask_bits, d.mask_batch = mask[0].data_ptr(), x.shape[0]
    elif dcode != L.F16 and Fp8.eligible(layer, x) and (not Fp8.copy_only() or Fp8.usable(src, layer, x, ldi)):
        # (a usable copy: the producer quantised act(x) with its tensor's scale)
        _attach_f8_operand(d, layer.prepared_f8, x, src if Fp8.usable(src, layer, x, ldi) else None, "fwd")
        if Fp8.PRODUCER and want_act is not None and not out_f32 and ldo % 64 == 0 and co_fill == ldo:
            eo = Fp8.site(layer.f8, "f8o", x.device, layer=layer)
            if eo is not None:
                # a post-activation output already holds want_act(out): its copy is the quantisation of the stored value
                assert not layer.out_act or layer.out_act == want_act
                d.out_f8_act = L.ACT_NONE if layer.out_act else want_act
                t8 = _attach_f8_copy(d, eo, out.shape, x.device, "fwd_copy_out")
                if t8 is not None:
                    side.f8_out = Fp8.handle(eo, t8, want_act)
    bits = None
    if side.want_bits and not out_f32 and out.dtype == torch.bfloat16 and ldo % 8 == 0:
        bits = torch.empty((n, ho, wo, ldo // 8), dtype=torch.uint8, device=x.device)
        d.sign_out = bits.data_ptr()
    assert round8(layer.ci_log) <= ldi, (layer.name, layer.ci_log, ldi)
    _launch_conv(d, layer, "fwd", 2.0 * n * ho * wo * layer.k * layer.k * layer.cin_v * layer.co)
    if bits is not None and L.load().ups_conv_sign_out_written():
        side.bits = bits                # (a launch that went to a kernel that does not write them hands none on: upsparts_hip.h)
    return out


def conv_dgrad(g, x, layer, res=None, mask_view=None, n_parts=0, f8_src="pop", x_bits=None):
    """gx = act'(x) * conv^T(g) (+ res);  g [n,ho,wo,ldg] in the activation dtype, x the forward input.
    mask_view (fp32 [B,hi,wi,3], with n_parts): the forward was the part-masked convolution; returns d loss / d hard
    [B,hi,wi,P] = sum_c gx[p*B+b,...,c] * view[b,...,c] straight from the kernel's epilogue (gx is never written).
    f8_src: the e5m2 copy of g its producer registered (ops.Fp8.grad_copy), None, or "pop" = look it up here.
    x_bits: the sign bytes of x its producer wrote ([n,hi,wi,ldi/8] uint8, ops.SignBits): read instead of x for act'."""
    n, hi, wi, ldi = x.shape
    if x_bits is not None and (tuple(x_bits.shape) != (n, hi, wi, ldi // 8) or layer.act_in == L.ACT_NONE):
        x_bits = None
    if SignBits.stats is not None and layer.act_in != L.ACT_NONE and mask_view is None:
        key = (layer.name, n, hi, wi, ldi, layer.k, layer.stride, x_bits is not None)
        SignBits.stats[key] = SignBits.stats.get(key, 0) + 1
    dcode = L.dt(x)
    ho, wo = layer.out_hw(hi, wi)
    ent = layer.prepared(dcode, hi, wi)
    g_hard = None
    if mask_view is not None:
        assert layer.stride == 1 and layer.act_in == L.ACT_NONE and res is None
        g_hard = torch.empty((n, hi, wi, n_parts), dtype=torch.float32, device=x.device)
        gx = None
        n_img = n * n_parts
    else:
        gx = torch.empty_like(x)
        n_img = n
    k, st = layer.k, layer.stride
    _, pby = same_geometry(hi, k, st)
    _, pbx = same_geometry(wi, k, st)
    cd2s = layer.d2s_channels(x) if mask_view is None else 0
    if cd2s:
        # one stride-1 3x3 convolution over the gradient lattice with 4 C channels (parity class, channel), written
        # depth-to-space: g is read once and whole output rows are stored (the per-class launches below store every other pixel)
        d = _conv_desc(dcode, g, (n, ho, wo, round8(layer.co), g.shape[-1]), layer.prepared_d2s(hi, wi)["w"], gx,
                       (ho, wo, 4 * cd2s, 4 * cd2s, ldi), ([t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)], range(9)),
                       3, 3, layer.slope, lattice=(hi, wi, 1, 0, 0))
        _attach_dgrad(d, layer, x, x_bits, res)
        d.d2s = cd2s
        _launch_conv(d, layer)
        return gx
    classes = [(0, 0)] if st == 1 else [(py, px) for py in range(st) for px in range(st)]
    for (py, px) in classes:
        lat_h = (hi - py + st - 1) // st
        lat_w = (wi - px + st - 1) // st
        if lat_h <= 0 or lat_w <= 0:
            continue
        dy, dx, tw = [], [], []
        for r in range(k):
            if (py + pby - r) % st:
                continue
            for s in range(k):
                if (px + pbx - s) % st:
                    continue
                dy.append((py + pby - r) // st); dx.append((px + pbx - s) // st); tw.append(r * k + s)
        if not dy:      # no tap reaches this parity class
            raise L.UpsError("empty tap class is not expected for k=3/k=1 'SAME' convolutions")
        d = _conv_desc(dcode, g, (n_img, ho, wo, round8(layer.co), g.shape[-1]), ent["w_dgrad"], gx,
                       (lat_h, lat_w, layer.ci_log, ldi, ldi), (dy, dx, tw), 1, len(dy), layer.slope, lattice=(hi, wi, st, py, px))
        _attach_dgrad(d, layer, x, x_bits, res)
        if mask_view is not None:
            d.mask_grad, d.mask_view, d.mask_batch = g_hard.data_ptr(), mask_view.data_ptr(), n
        elif st == 1 and Fp8.enabled and Fp8.GRAD and g.dtype == torch.bfloat16:
            src = Fp8.grad_copy(g) if isinstance(f8_src, str) else f8_src
            use_f8 = Fp8.eligible_grad(layer, g, x)
            src_ok = use_f8 and src is not None and layer.ci_log > 32 and g.shape[-1] % 16 == 0
            emit = False
            if use_f8 and (src_ok or not Fp8.copy_only()):
                # (a copy in hand: the producer wrote e5m2(g * scale) in its epilogue)
                _attach_f8_operand(d, layer.prepared_f8_grad, g, src if src_ok else None, "dgrad")
                d.f8_e5m2 = 1
                emit = True
            elif layer.k == 3 and round8(layer.co) <= 32 and hi % 16 == 0 and wi % 16 == 0:
                emit = True     # a bf16 launch off the 128-wide two-blocks-per-CU instance (the P-channel head): it can write the copy
            if emit and Fp8.PRODUCER and gx is not None and ldi % 64 == 0 and layer.ci_log == ldi:
                eo = Fp8.site(layer.f8, "f8go", x.device, e5m2=True, layer=layer)
                if eo is not None:
                    d.out_f8_act, d.out_f8_e5m2 = L.ACT_NONE, 1
                    t8 = _attach_f8_copy(d, eo, gx.shape, x.device, "dgrad_copy_out")
                    if t8 is not None:
                        Fp8.register_grad_copy(gx, Fp8.handle(eo, t8))
        assert round8(layer.co) <= g.shape[-1]
        _launch_conv(d, layer, "dgrad" if st == 1 else None)
    return gx if mask_view is None else g_hard


COORD_STREAM = SW.flag("UPS_COORD_STREAM")     # A/B switch: CoordConv rows of the weight gradients on their own stream


def conv_wgrad(g, x, layer, mask=None, fmt=None, launch_stream=None, f8_src=None):
    """(dV [kh,kw,cin_v,co] fp32, db [co] fp32).  mask = (hard_bits, P): x is the unmasked view of a part-masked convolution.
    fmt = L.F16: x holds fp16 (converted to bf16, the gradient's type, while it is staged).
    launch_stream: the stream whose position marks "g and x are ready" when the call itself runs on the weight-gradient side stream:
    the CoordConv rows (batch sum of g + two small kernels: they write rows of dV the main kernel does not touch) then go to a
    second side stream, beside the layer's main weight-gradient kernel instead of behind it -- the weight-gradient stream is a
    serial chain that ends the step (tools/timeline.py), and these ~40 small launches were 1 ms of it.
    f8_src: the e5m2 copy of g (the handle ops.Fp8.grad_copy returns): the wide 3x3 / stride-1 layers then run on the fp8 kernel
    (ups_wgrad_desc.dout_f8; x is quantised while it is staged, with this layer's delayed scale)."""
    n, hi, wi, ldi = x.shape
    if mask is not None:
        n = n * mask[1]
    dcode = L.dt(x)
    ho, wo = layer.out_hw(hi, wi)
    dev = x.device
    gV = layer.grad_V if layer.grad_V is not None else torch.empty_like(layer.V)
    gb = layer.grad_b if layer.grad_b is not None else torch.empty_like(layer.b)
    d = L.WgradDesc()
    d.dtype = dcode
    d.n, d.hi, d.wi, d.ci, d.ldi = n, hi, wi, round8(layer.ci_log), ldi
    d.ci_log, d.cin_v = layer.ci_log, layer.cin_v
    d.ho, d.wo, d.co, d.ldo = ho, wo, layer.co, g.shape[-1]
    d.in_sy = d.in_sx = layer.stride
    dy, dx, tw = layer.fwd_taps(hi, wi)
    _fill_taps(d, dy, dx, tw, layer.k * layer.k)
    d.act_in, d.act_slope = (L.ACT_NONE if layer.in_post else layer.act_in), layer.slope
    sk, wsb = C.c_int32(0), C.c_size_t(0)
    d.in_, d.dout, d.grad, d.grad_bias = x.data_ptr(), g.data_ptr(), gV.data_ptr(), gb.data_ptr()
    if mask is not None:
        d.mask_bits, d.mask_batch = mask[0].data_ptr(), x.shape[0]
    d.in_f16 = int(fmt == L.F16)
    if f8_src is not None and f8_src.get("t") is not None and Fp8.eligible_wgrad(layer, g, x, mask) \
            and tuple(f8_src["t"].shape) == tuple(g.shape):
        ew = layer.prepared_f8_wgrad(x, fmt)
        d.dout_f8 = f8_src["t"].data_ptr()
        d.dout_f8_scale = Fp8.scale[f8_src["slot"]:].data_ptr()
        d.in_f8_scale = Fp8.scale[ew["slot"]:].data_ptr()
        d.in_f8_amax = Fp8.amax[ew["slot"]].data_ptr()
        Fp8.stats["wgrad_f8"] += 1
        Fp8.mark_used(f8_src)
    L.call("ups_conv_wgrad_plan", C.byref(d), C.byref(sk), C.byref(wsb))
    ws = WORKSPACE.get(wsb.value, dev)
    d.splitk, d.workspace = sk.value, ws.data_ptr()
    L.call("ups_conv_wgrad", C.byref(d), L.stream())        # dV (main channels) + db from the same dout tiles
    if layer.coords:
        def coord_rows():
            gsum = torch.empty((ho * wo, layer.co), dtype=torch.float32, device=dev)
            L.call("ups_batch_sum", L.ptr(g), dcode, n, ho * wo, layer.co, g.shape[-1], L.ptr(gsum), L.stream())
            ax, ay = 2.0 / max(1, hi - 1), 2.0 / max(1, wi - 1)
            scratch = COLSUM_WS.get((layer.k + 1) * 2 * wo * layer.co * 4, dev)
            L.call("ups_coord_wgrad", L.ptr(gsum), hi, wi, ho, wo, layer.co, layer.k, layer.k,
                   (C.c_int32 * 9)(*dy), (C.c_int32 * 9)(*dx), layer.stride, layer.stride, ax, ay,
                   layer.ci_log, L.ptr(gV), None, L.ptr(scratch), L.stream())
        if launch_stream is not None and COORD_STREAM and Streams.enabled:
            s2 = Streams.get("wgrad2", dev)
            s2.wait_stream(launch_stream)
            with torch.cuda.stream(s2):
                coord_rows()
        else:
            coord_rows()
    return gV, gb


def to_act_dtype(g, like_dtype, co):
    """fp32 gradient [.., c] of an fp32-output conv -> activation dtype with 8-padded channels."""
    ld = round8(co)
    if g.dtype == like_dtype and g.shape[-1] == ld:
        return g.contiguous()
    g = g.contiguous()
    assert g.dtype == torch.float32
    out = torch.empty(g.shape[:-1] + (ld,), dtype=like_dtype, device=g.device)
    rows = g.numel() // g.shape[-1]
    L.call("ups_pad_convert", L.ptr(g), g.shape[-1], L.ptr(out), L.dt(out), ld, rows, L.stream())
    return out


class GradMode(object):
    """ctx.needs_input_grad is fixed when the tape is recorded, not per autograd.grad call; a backward pass
    that only wants input gradients (e.g. d rec / d z through the mask decoder) sets skip_wgrad."""
    skip_wgrad = False


class skip_wgrad(object):
    def __enter__(self):
        self.prev, GradMode.skip_wgrad = GradMode.skip_wgrad, True

    def __exit__(self, *a):
        GradMode.skip_wgrad = self.prev


class ConvFn(torch.autograd.Function):
    """res_mode 0: plain; 1: out = res + conv(x); 2: out = x + conv(act(x)) (residual_block, nn.py:1042-1056)."""

    @staticmethod
    def forward(ctx, x, V, b, res, layer, res_mode, out_f32, ldo, hard=None, hard_bits=None, view_f32=None, fmt=None, res_post=False,
                x_bits=None, side=None):
        """hard / hard_bits / view_f32 given: the part-masked convolution (x = the unmasked view in the activation dtype,
        the P*B part images are formed in the kernel's load); the gradient w.r.t. `hard` comes out of the dgrad epilogue.
        side: the call's Handoff; it goes to conv_forward and is not kept on ctx (the tape pins neither fp8 copy nor sign bytes)."""
        x = x.contiguous()
        r = x if res_mode == 2 else (res.contiguous() if res_mode == 1 else None)
        ctx.mask = None if hard is None else (hard_bits, hard.shape[-1])
        # res_mode 2: the residual is the input itself -- stored post-activation exactly when the layer's input is
        out = conv_forward(x, layer, res=r, out_f32=out_f32, ldo=ldo, mask=ctx.mask, fmt=fmt,
                           res_post=layer.in_post if res_mode == 2 else bool(res_post), side=side)
        ctx.save_for_backward(x, view_f32)
        ctx.layer, ctx.res_mode, ctx.fmt = layer, res_mode, fmt
        ctx.x_bits = x_bits             # sign bytes of x from its producer (SignBits): the input gradient reads them instead of x
        return out

    @staticmethod
    def backward(ctx, g):
        x, view_f32 = ctx.saved_tensors
        layer = ctx.layer
        g = to_act_dtype(g, x.dtype, layer.co)
        gx = gV = gb = gres = g_hard = None
        offloaded = False
        # the e5m2 copy of g its producer wrote (fp8 mode): looked up ONCE, read by the weight gradient and by the input gradient
        f8_src = Fp8.grad_copy(g) if (Fp8.enabled and Fp8.GRAD and ctx.mask is None and layer.stride == 1
                                      and g.dtype == torch.bfloat16) else None
        if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and not GradMode.skip_wgrad:
            if Streams.enabled and layer.grad_V is not None and not Streams.on_aux(x.device):
                offloaded = True
                # weight gradient on the side stream (it lands in the layer's view of the flat gradient bucket, which
                # nothing reads before Streams.join); g and x must outlive the side stream's reads
                cur = torch.cuda.current_stream(x.device)
                side = Streams.get("wgrad", x.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    gV, gb = conv_wgrad(g, x, layer, mask=ctx.mask, fmt=ctx.fmt, launch_stream=cur, f8_src=f8_src)
                Streams.keep(x.device, g, x)      # alive until the launching stream has joined the side stream(s)
                if f8_src is not None:
                    Streams.keep(x.device, f8_src["t"])
            else:
                gV, gb = conv_wgrad(g, x, layer, mask=ctx.mask, fmt=ctx.fmt, f8_src=f8_src)
            if layer.after_wgrad is not None:
                layer.after_wgrad()
        if ctx.mask is not None:
            if ctx.needs_input_grad[8]:
                g_hard = conv_dgrad(g, x, layer, mask_view=view_f32, n_parts=ctx.mask[1])
        elif ctx.needs_input_grad[0]:
            gx = conv_dgrad(g, x, layer, res=g if ctx.res_mode == 2 else None, f8_src=f8_src if layer.stride == 1 else "pop",
                            x_bits=ctx.x_bits)
        if ctx.res_mode == 1 and ctx.needs_input_grad[3]:
            # the autograd engine may accumulate other branches into the returned tensor IN PLACE; the side stream
            # is still reading g, so hand out a copy in that case
            gres = g.clone() if offloaded else g
        return gx, gV, gb, gres, None, None, None, None, g_hard, None, None, None, None, None, None


def conv(x, layer, res=None, res_self=False, out_f32=False, ldo=None, mask=None, fmt=None, res_post=False, x_bits=None, side=None):
    """mask = (hard [B,H,W,P] fp32 autograd leaf, hard_bits [B,H,W] int32, view_f32 [B,H,W,3]): part-masked convolution.
    res_post: `res` is stored post-activation (ups_conv_desc.res_act).  x_bits: the sign bytes of x (SignBits).
    side: this call's Handoff -- the input's fp8 copy, what is wanted of the output, and what the call wrote."""
    mode = 2 if res_self else (1 if res is not None else 0)
    if mask is None:
        return ConvFn.apply(x, layer.V, layer.b, res, layer, mode, out_f32, ldo, None, None, None, fmt, res_post, x_bits, side)
    assert mode == 0
    return ConvFn.apply(x, layer.V, layer.b, None, layer, 0, out_f32, ldo, mask[0], mask[1], mask[2].contiguous(), None, False, None,
                        side)


# ---------------------------------------------------------------------------------------------------------------------------------
# upsample(x, nf, "conv_transposed"): weight-normalised deconv2d, 3x3 / stride 2 / 'SAME' (nn.py:818-822, 938-1039; csrc/deconv3x3_s2.hip)
DECONV_ONE_LAUNCH = True        # False: the forward as four per-class ups_conv_igemm launches (tools/bench_deconv.py, parity tests)
# the four output parity classes: taps (k, source offset) of an even / odd output row (or column) -- r-major in the class launches
_DECONV_TAPS = {0: ((0, 0), (2, -1)), 1: ((1, 0),)}


class DeconvLayer(_Layer):
    """One deconv2d variable triple: V [3,3,nf,Cin(+2)] (TF transpose layout [kh, kw, out, in]), g [nf], b [nf].  The layer is
    the input gradient of a stride-2 3x3 convolution with forward weights W = g * l2_normalize(V): its forward is four parity
    classes of taps, dx a stride-2 forward convolution of dy with W, dW a stride-2 weight gradient with the two tensors' roles
    swapped.  W's operands are a WeightCopy made by ups_deconv_prep: like every copy of a trainable layer it is re-made by the
    model's PrepRegistry behind Adam, in a captured step too."""

    def __init__(self, name, V, g, b, coords):
        _Layer.__init__(self, name, V)
        self.g, self.b, self.coords = g, b, coords
        self.co = V.shape[2]
        self.cin_v = V.shape[3]
        self.ci_log = self.cin_v - (2 if coords else 0)
        self.grad_V = self.grad_g = self.grad_b = None     # optional views into the flat gradient bucket

    def prepared(self, fwd_code, dx_code, hi, wi):
        """W's operands for an hi x wi input: forward (fwd_code), input gradient (dx_code), fp32 W, 1 / ||V_o||, CoordConv tables."""
        key = ("deconv", fwd_code, dx_code, hi, wi)
        copy = self.copies.get(key)
        if copy is None:
            dev = self.V.device
            bkf, bkd = (16 if fwd_code == L.F32 else 32), (16 if dx_code == L.F32 else 32)
            ent = {"w_fwd": torch.empty((9, -(-round8(self.ci_log) // bkf), self.co, bkf), dtype=L.torch_dtype(fwd_code), device=dev),
                   "w_dx": torch.empty((9, -(-round8(self.co) // bkd), self.ci_log, bkd), dtype=L.torch_dtype(dx_code), device=dev),
                   "w32": torch.empty_like(self.V), "inv": torch.empty((self.co,), dtype=torch.float32, device=dev),
                   "ctab": torch.empty((4, 64, 3, self.co), dtype=torch.float32, device=dev) if self.coords else None}
            copy = self.copies[key] = WeightCopy(self, ent, lambda: L.call(
                "ups_deconv_prep", L.ptr(self.V), L.ptr(self.g), self.co, self.cin_v, self.ci_log, fwd_code, L.ptr(ent["w_fwd"]),
                dx_code, L.ptr(ent["w_dx"]), L.ptr(ent["w32"]), L.ptr(ent["inv"]), L.ptr(ent["ctab"]), hi, wi, L.stream()))
        return copy.get()


def _dx_code(x):
    return L.F32 if x.dtype == torch.float32 else L.BF16


def deconv_forward(x, layer, fmt=None, one_launch=None):
    """y [n, 2hi, 2wi, round8(nf)] = deconv(x (+coords), W) + b; x [n, hi, wi, ldi].  fmt = L.F16: x and y hold fp16 (bf16 containers).
    16-bit tensors go to the one-launch kernel (ups_deconv3x3_s2_fwd) where it takes the shape, everything else to four per-class
    launches of the convolution engine (the per-class input-gradient launches of conv_dgrad, fed with W, bias and class tables)."""
    n, hi, wi, ldi = x.shape
    fcode = L.dt(x) if fmt is None else fmt
    assert fcode != L.F16 or x.dtype == torch.bfloat16
    ent = layer.prepared(fcode, _dx_code(x), hi, wi)
    nf, ci, ldo = layer.co, round8(layer.ci_log), round8(layer.co)
    assert ci <= ldi, (layer.name, layer.ci_log, ldi)
    out = torch.empty((n, 2 * hi, 2 * wi, ldo), dtype=x.dtype, device=x.device)
    ctab = ent["ctab"]
    one_launch = DECONV_ONE_LAUNCH if one_launch is None else one_launch
    if one_launch and fcode != L.F32:
        rc = L.load().ups_deconv3x3_s2_fwd(L.ptr(x), fcode, n, hi, wi, ci, ldi, L.ptr(ent["w_fwd"]), L.ptr(layer.b), L.ptr(ctab),
                                           nf, ldo, L.ptr(out), L.stream())
        if rc == 0:
            return out
        if rc != -2:            # UPS_E_UNSUPPORTED: nothing launched, the shape goes to the class launches
            L.check(rc, "ups_deconv3x3_s2_fwd")
    for py in (0, 1):
        for px in (0, 1):
            dy, dx, tw = [], [], []
            for ky, oy in _DECONV_TAPS[py]:
                for kx, ox in _DECONV_TAPS[px]:
                    dy.append(oy); dx.append(ox); tw.append(3 * ky + kx)
            d = _conv_desc(fcode, x, (n, hi, wi, ci, ldi), ent["w_fwd"], out, (hi, wi, nf, ldo, ldo), (dy, dx, tw),
                           len(_DECONV_TAPS[py]), len(_DECONV_TAPS[px]), 0.2, lattice=(2 * hi, 2 * wi, 2, py, px))
            d.bias = layer.b.data_ptr()
            d.coord_tab = ctab[2 * py + px].data_ptr() if ctab is not None else None
            _launch_conv(d, layer)
    return out


def deconv_dgrad(g, x, layer, fmt=None):
    """dx = conv2d(dy, W[.., :Cin], stride 2, 'SAME') -- a forward launch of the convolution engine (the stride-2 kernels where their
    gates admit the shape).  g [n, 2hi, 2wi, ldg] in the gradient dtype."""
    n, hi, wi, ldi = x.shape
    ent = _deconv_ent(layer, x, fmt)
    gx = torch.empty_like(x)
    assert round8(layer.co) <= g.shape[-1]
    d = _conv_desc(_dx_code(x), g, (n, 2 * hi, 2 * wi, round8(layer.co), g.shape[-1]), ent["w_dx"], gx, (hi, wi, layer.ci_log, ldi, ldi),
                   ([t // 3 for t in range(9)], [t % 3 for t in range(9)], range(9)), 3, 3, 0.2, in_stride=2)   # pad 0 before (even 2hi)
    _launch_conv(d, layer)
    return gx


def _deconv_ent(layer, x, fmt):
    """The entry the forward of this input used."""
    copy = layer.copies.get(("deconv", L.dt(x) if fmt is None else fmt, _dx_code(x)) + tuple(x.shape[1:3]))
    if copy is not None:
        return copy.bufs
    raise L.UpsError("{}: no prepared deconvolution weights for input {}".format(layer.name, tuple(x.shape)))


def deconv_wgrad(g, x, layer, fmt=None):
    """(dV, dg, db): dW[.., :Cin] from the stride-2 weight-gradient kernel with dy as the convolution's input and x as its output
    gradient, dW's coordinate columns and db from ups_deconv_bias_coord_grad, then (dV, dg) through the normalisation."""
    n, hi, wi, ldi = x.shape
    dev = x.device
    nf, ci_log = layer.co, layer.ci_log
    gV = layer.grad_V if layer.grad_V is not None else torch.empty_like(layer.V)
    gg = layer.grad_g if layer.grad_g is not None else torch.empty_like(layer.g)
    gb = layer.grad_b if layer.grad_b is not None else torch.empty_like(layer.b)
    if fmt == L.F16:            # fp16 forward input (bf16 container): the weight-gradient kernel stages its output gradient as bf16
        xb = torch.empty_like(x)
        L.call("ups_convert", L.ptr(x), L.F16, L.ptr(xb), L.BF16, x.numel(), L.stream())
        x = xb
    dwx = torch.empty((3, 3, nf, ci_log), dtype=torch.float32, device=dev)
    d = L.WgradDesc()
    d.dtype = _dx_code(x)
    d.n, d.hi, d.wi, d.ci, d.ldi = n, 2 * hi, 2 * wi, round8(nf), g.shape[-1]
    d.ci_log, d.cin_v = nf, nf
    d.ho, d.wo, d.co, d.ldo = hi, wi, ci_log, ldi
    d.in_sy = d.in_sx = 2
    _fill_taps(d, [t // 3 for t in range(9)], [t % 3 for t in range(9)], list(range(9)), 9)
    d.act_in, d.act_slope = L.ACT_NONE, 0.2
    sk, wsb = C.c_int32(0), C.c_size_t(0)
    scratch_b = torch.empty((ci_log,), dtype=torch.float32, device=dev)     # (the swapped form's "bias" gradient: unused)
    d.in_, d.dout, d.grad, d.grad_bias = g.data_ptr(), x.data_ptr(), dwx.data_ptr(), scratch_b.data_ptr()
    L.call("ups_conv_wgrad_plan", C.byref(d), C.byref(sk), C.byref(wsb))
    ws = WORKSPACE.get(wsb.value, dev)
    d.splitk, d.workspace = sk.value, ws.data_ptr()
    L.call("ups_conv_wgrad", C.byref(d), L.stream())
    splits = max(1, min(256, n * 2 * hi))
    part = torch.empty((splits * 19 * nf,), dtype=torch.float32, device=dev)
    dwc = torch.empty((3, 3, nf, 2), dtype=torch.float32, device=dev) if layer.coords else None
    L.call("ups_deconv_bias_coord_grad", L.ptr(g), _dx_code(g), n, hi, wi, nf, g.shape[-1], int(layer.coords), L.ptr(gb), L.ptr(dwc),
           L.ptr(part), splits, L.stream())
    L.call("ups_deconv_wn_bwd", L.ptr(layer.V), L.ptr(layer.g), L.ptr(dwx), L.ptr(dwc), nf, layer.cin_v, ci_log, L.ptr(gV), L.ptr(gg),
           L.stream())
    return gV, gg, gb


class DeconvFn(torch.autograd.Function):
    """Autograd node of DeconvLayer: the weight gradients land in the layer's views of the flat gradient bucket, enqueued on the
    weight-gradient side stream like ConvFn's (skip_wgrad passes leave them alone)."""

    @staticmethod
    def forward(ctx, x, V, g, b, layer, fmt=None):
        x = x.contiguous()
        out = deconv_forward(x, layer, fmt=fmt)
        ctx.save_for_backward(x)
        ctx.layer, ctx.fmt = layer, fmt
        return out

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        layer = ctx.layer
        gy = to_act_dtype(gy, x.dtype, layer.co)
        gx = gV = gg = gb = None
        if any(ctx.needs_input_grad[1:4]) and not GradMode.skip_wgrad:
            if Streams.enabled and layer.grad_V is not None and not Streams.on_aux(x.device):
                cur = torch.cuda.current_stream(x.device)
                side = Streams.get("wgrad", x.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    gV, gg, gb = deconv_wgrad(gy, x, layer, fmt=ctx.fmt)
                Streams.keep(x.device, gy, x)
            else:
                gV, gg, gb = deconv_wgrad(gy, x, layer, fmt=ctx.fmt)
            if layer.after_wgrad is not None:
                layer.after_wgrad()
        if ctx.needs_input_grad[0]:
            gx = deconv_dgrad(gy, x, layer, fmt=ctx.fmt)
        return gx, gV, gg, gb, None, None


def deconv(x, layer, fmt=None):
    return DeconvFn.apply(x, layer.V, layer.g, layer.b, layer, fmt)


def masked_conv_eligible(dtype, size, n_parts):
    """The fused form runs on the bf16 3x3 / stride-1 patch kernels: 16-aligned images, at most 32 parts."""
    return dtype == torch.bfloat16 and size % 16 == 0 and size >= 16 and n_parts <= 32


class BilinearFn(torch.autograd.Function):
    """site: per-call-site state (a dict owned by the Scope) when the up-sampling feeds fp8 convolutions: its forward then also
    writes the e4m3 copy of act(y), its backward the e5m2 copy of the gradient it returns.  side: the call's Handoff (not kept on
    ctx) -- the forward leaves that copy in ``side.f8_out`` and, asked by ``side.want_bits``, a post-activation result's sign bytes
    in ``side.bits``."""

    @staticmethod
    def forward(ctx, x, site=None, act=0, slope=0.2, fmt=None, out_act=0, side=None):
        """out_act: the result is stored as out_act(y) (post-activation storage for a consuming residual block; gradients stay
        with respect to y, so the backward is unchanged).  `site` with an fp16 / post-activation forward (the mask decoder in fp8
        mode: its forward stays fp16, round 4): only the BACKWARD hands an e5m2 copy of the gradient on."""
        x = x.contiguous()
        n, h, w, c = x.shape
        y = torch.empty((n, 2 * h, 2 * w, c), dtype=x.dtype, device=x.device)
        f8_site = site is not None and Fp8.enabled and Fp8.PRODUCER and x.dtype == torch.bfloat16 and c % 64 == 0 and (2 * h) % 16 == 0
        ctx.site, ctx.shape = (site if f8_site else None), (n, h, w, c)
        if out_act:
            if side is not None and side.want_bits and x.dtype == torch.bfloat16 and c % 8 == 0:
                side.bits = torch.empty((n, 2 * h, 2 * w, c // 8), dtype=torch.uint8, device=x.device)
                L.call("ups_bilinear2x_fwd_bits", L.ptr(x), L.ptr(y), L.dt(x) if fmt is None else fmt, n, h, w, c, out_act, slope,
                       L.ptr(side.bits), L.stream())
            else:
                L.call("ups_bilinear2x_fwd_act", L.ptr(x), L.ptr(y), L.dt(x) if fmt is None else fmt, n, h, w, c, out_act, slope, L.stream())
            return y
        so = Fp8.site(site, "fwd", x.device) if (f8_site and fmt != L.F16) else None
        if so is not None:
            t8 = Fp8.emit(so, y.shape, x.device)
            L.call("ups_bilinear2x_fwd_f8", L.ptr(x), L.ptr(y), n, h, w, c, L.ptr(t8),
                   L.ptr(Fp8.scale[so["slot"]:]), L.ptr(Fp8.amax[so["slot"]]), act, slope, 0, L.stream())
            if side is not None and t8 is not None:
                side.f8_out = Fp8.handle(so, t8, act)
        else:
            L.call("ups_bilinear2x_fwd", L.ptr(x), L.ptr(y), L.dt(x) if fmt is None else fmt, n, h, w, c, L.stream())
        return y

    @staticmethod
    def backward(ctx, g):
        n, h, w, c = ctx.shape
        g = g.contiguous()
        gx = torch.empty((n, h, w, c), dtype=g.dtype, device=g.device)
        site = ctx.site
        so = None
        if site is not None and Fp8.GRAD and g.dtype == torch.bfloat16 and h % 16 == 0:
            so = Fp8.site(site, "bwd", g.device, e5m2=True)
        if so is not None:
            t8 = Fp8.emit(so, gx.shape, g.device)
            L.call("ups_bilinear2x_bwd_f8", L.ptr(g), L.ptr(gx), n, h, w, c, L.ptr(t8),
                   L.ptr(Fp8.scale[so["slot"]:]), L.ptr(Fp8.amax[so["slot"]]), 1, L.stream())
            if t8 is not None:
                Fp8.register_grad_copy(gx, Fp8.handle(so, t8))
        else:
            L.call("ups_bilinear2x_bwd", L.ptr(g), L.ptr(gx), L.dt(g), n, h, w, c, L.stream())
        return gx, None, None, None, None, None, None


class DepthToSpaceFn(torch.autograd.Function):
    """tf.depth_to_space(x, 2) of the "subpixel" up-sampling (nn.py:824-827): [n,h,w,ld(4C)] -> [n,2h,2w,round8(C)]."""

    @staticmethod
    def forward(ctx, x, C, fmt=None):
        x = x.contiguous()
        n, h, w, ldx = x.shape
        y = torch.empty((n, 2 * h, 2 * w, round8(C)), dtype=x.dtype, device=x.device)
        L.call("ups_depth_to_space", L.ptr(x), L.ptr(y), L.dt(x) if fmt is None else fmt, n, h, w, C, ldx, y.shape[-1], 0, L.stream())
        ctx.dims = (n, h, w, C, ldx)
        return y

    @staticmethod
    def backward(ctx, g):
        n, h, w, C, ldx = ctx.dims
        g = g.contiguous()
        gx = torch.empty((n, h, w, ldx), dtype=g.dtype, device=g.device)
        L.call("ups_depth_to_space", L.ptr(g), L.ptr(gx), L.dt(g), n, h, w, C, ldx, g.shape[-1], 1, L.stream())
        return gx, None, None


class Nearest2xFn(torch.autograd.Function):
    """tf.image.resize_images(NEAREST_NEIGHBOR) to twice the size (nn.py:828-833): every pixel repeated 2x2."""

    @staticmethod
    def forward(ctx, x, fmt=None):
        x = x.contiguous()
        n, h, w, c = x.shape
        y = torch.empty((n, 2 * h, 2 * w, c), dtype=x.dtype, device=x.device)
        L.call("ups_nearest2x", L.ptr(x), L.ptr(y), L.dt(x) if fmt is None else fmt, n, h, w, c, 0, L.stream())
        ctx.dims = (n, h, w, c)
        return y

    @staticmethod
    def backward(ctx, g):
        n, h, w, c = ctx.dims
        g = g.contiguous()
        gx = torch.empty((n, h, w, c), dtype=g.dtype, device=g.device)
        L.call("ups_nearest2x", L.ptr(g), L.ptr(gx), L.dt(g), n, h, w, c, 1, L.stream())
        return gx, None


class CropFn(torch.autograd.Function):
    """The ho x wo window of an NHWC tensor at the corner held in `yx` (int32 [2] ON THE DEVICE: no host sync, valid inside a
    captured HIP graph) -- `perceptual_input: resize256_crop224` (Trainer)."""

    @staticmethod
    def forward(ctx, x, yx, ho, wo):
        x = x.contiguous()
        n, h, w, c = x.shape
        assert yx.dtype == torch.int32 and yx.numel() == 2 and yx.is_cuda
        y = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
        L.call("ups_crop_fwd", L.ptr(x), L.ptr(y), L.dt(x), n, h, w, c, ho, wo, L.ptr(yx), L.stream())
        ctx.save_for_backward(yx)
        ctx.shape = (n, h, w, c)
        return y

    @staticmethod
    def backward(ctx, g):
        (yx,) = ctx.saved_tensors
        n, h, w, c = ctx.shape
        g = g.contiguous()
        gx = torch.empty((n, h, w, c), dtype=g.dtype, device=g.device)
        L.call("ups_crop_bwd", L.ptr(g), L.ptr(gx), L.dt(g), n, h, w, c, g.shape[1], g.shape[2], L.ptr(yx), L.stream())
        return gx, None, None, None


class ActMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, slope, post=False):
        """post: x already holds act(x) (post-activation storage): plain mean forward, act' from its sign backward."""
        x = x.contiguous()
        n, h, w, c = x.shape
        y = torch.empty((n, 1, 1, c), dtype=x.dtype, device=x.device)
        L.call("ups_act_mean_fwd", L.ptr(x), L.ptr(y), L.dt(x), n, h * w, c, L.ACT_NONE if post else act, slope, L.stream())
        ctx.save_for_backward(x)
        ctx.act, ctx.slope = act, slope
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        n, h, w, c = x.shape
        g = g.contiguous()
        gx = torch.empty_like(x)
        L.call("ups_act_mean_bwd", L.ptr(x), L.ptr(g), L.ptr(gx), L.dt(x), n, h * w, c, ctx.act, ctx.slope, L.stream())
        return gx, None, None, None


class EluFn(torch.autograd.Function):
    """activate(x, "elu") (nn.py:747-758): the one activation that is materialised -- the convolution kernels fuse only the
    max(x, slope * x) family into their loads; a scope with `activation: elu` (no shipped yaml) runs its convolutions on the
    activated tensor.  fmt = L.F16: fp16 bits in a bf16 container."""

    @staticmethod
    def forward(ctx, x, fmt=None):
        x = x.contiguous()
        y = torch.empty_like(x)
        ctx.dcode = L.dt(x) if fmt is None else fmt
        L.call("ups_elu_fwd", L.ptr(x), L.ptr(y), ctx.dcode, x.numel(), L.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()
        gx = torch.empty_like(x)
        # (gradients of fp16 forward tensors are bf16: the derivative is taken in the gradient's type from the fp16 input)
        if ctx.dcode == L.F16:
            xb = x.view(torch.float16).to(torch.bfloat16)
            L.call("ups_elu_bwd", L.ptr(xb), L.ptr(g), L.ptr(gx), L.BF16, x.numel(), L.stream())
        else:
            L.call("ups_elu_bwd", L.ptr(x), L.ptr(g), L.ptr(gx), ctx.dcode, x.numel(), L.stream())
        return gx, None


class MaxPoolFn(torch.autograd.Function):
    """site (fp8 mode): per-call-site state when the pooled tensor feeds an fp8 convolution -- the forward then also writes the
    e4m3 copy of act(y) (Fp8State.site / emit) and leaves it in ``side.f8_out`` (side: the call's Handoff, not kept on ctx);
    `act` = the activation-on-load of that consumer."""

    @staticmethod
    def forward(ctx, x, site=None, act=0, side=None):
        x = x.contiguous()
        n, h, w, c = x.shape
        y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
        f8 = (site is not None and Fp8.enabled and Fp8.PRODUCER and x.dtype == torch.bfloat16 and c % 64 == 0
              and (h // 2) % 16 == 0 and (w // 2) % 16 == 0)
        so = Fp8.site(site, "fwd", x.device) if f8 else None
        if so is not None:
            t8 = Fp8.emit(so, y.shape, x.device)
            L.call("ups_maxpool2_fwd_f8", L.ptr(x), L.ptr(y), n, h, w, c, L.ptr(t8),
                   L.ptr(Fp8.scale[so["slot"]:]), L.ptr(Fp8.amax[so["slot"]]), act, 0.2, L.stream())
            if side is not None and t8 is not None:
                side.f8_out = Fp8.handle(so, t8, act)
        else:
            L.call("ups_maxpool2_fwd", L.ptr(x), L.ptr(y), L.dt(x), n, h, w, c, L.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        n, h, w, c = x.shape
        g = g.contiguous()
        gx = torch.empty_like(x)
        L.call("ups_maxpool2_bwd", L.ptr(x), L.ptr(g), L.ptr(gx), L.dt(x), n, h, w, c, L.stream())
        return gx, None, None, None


class VggPreFn(torch.autograd.Function):
    """[-1,1] RGB -> BGR*255 - ImageNet mean, 8-channel padded (edflow VGG19Features, UNVERIFIED)."""

    @staticmethod
    def forward(ctx, x, act_dtype):
        x = x.contiguous()
        pixels = x.numel() // x.shape[-1]
        y = torch.empty(x.shape[:-1] + (8,), dtype=act_dtype, device=x.device)
        L.call("ups_vgg_preprocess_fwd", L.ptr(x), int(x.dtype == torch.float32), x.shape[-1], L.ptr(y), L.dt(y),
               pixels, L.stream())
        ctx.in_shape, ctx.in_dtype = x.shape, x.dtype
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        assert ctx.in_dtype == g.dtype, "gradient flows back to an activation-dtype image"
        gx = torch.empty(ctx.in_shape, dtype=g.dtype, device=g.device)
        L.call("ups_vgg_preprocess_bwd", L.ptr(g), L.ptr(gx), L.dt(g), ctx.in_shape[-1],
               g.numel() // 8, L.stream())
        return gx, None


L1_BLOCKS = 1024


class L1MeanFn(torch.autograd.Function):
    """mean |act(a) - act(b)| over the logical channels; gradient w.r.t. b only (a is the target)."""

    @staticmethod
    def forward(ctx, a, b, c_log, act):
        a, b = a.contiguous(), b.contiguous()
        rows, ld = b.numel() // b.shape[-1], b.shape[-1]
        partial = torch.empty(L1_BLOCKS, dtype=torch.float32, device=b.device)
        out = torch.empty((), dtype=torch.float32, device=b.device)
        L.call("ups_l1_fwd", L.ptr(a), L.ptr(b), L.dt(b), rows, c_log, ld, act, L.ptr(partial), L1_BLOCKS, L.stream())
        L.call("ups_sum_scale", L.ptr(partial), L1_BLOCKS, 1.0 / (rows * c_log), L.ptr(out), 0, L.stream())
        ctx.save_for_backward(a, b)
        ctx.c_log, ctx.act = c_log, act
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        rows, ld = b.numel() // b.shape[-1], b.shape[-1]
        gb = torch.empty_like(b)
        g = g.contiguous().float()
        L.call("ups_l1_bwd", L.ptr(a), L.ptr(b), L.ptr(gb), L.dt(b), rows, ctx.c_log, ld, ctx.act, L.ptr(g),
               1.0 / (rows * ctx.c_log), L.stream())
        return None, gb, None, None


# G(F)[b] = F[b]^T F[b] / (GRAM_DIV * h * w): edflow VGG19Features' Gram normalisation as recalled (UNVERIFIED; tests/gram_ref.py
# restates the same constant)
GRAM_DIV = 4.0
_GRAM_PLANS = {}


def gram_plan(n, hw, c, dtype):
    """(K splits, partial floats, workspace floats, sign bytes) of ups_gram_l1_fwd at this shape (cached: one C call per shape)."""
    key = (n, hw, c, dtype)
    if key not in _GRAM_PLANS:
        out = (C.c_int64 * 4)()
        L.check(L.load().ups_gram_plan(n, hw, c, dtype, out), "ups_gram_plan")
        _GRAM_PLANS[key] = tuple(int(v) for v in out)
    return _GRAM_PLANS[key]


class PerceptualTermFn(torch.autograd.Function):
    """One feature map's perceptual term with edflow's Gram term: mean |act(a) - act(b)| + gram_w * mean_{b,i,j} |G(a) - G(b)|
    (a, b [n,h,w,ld], G over the c logical channels of act(.)); gradient w.r.t. b only (a is the target).  The L1 kernels write the
    term and its gradient, the Gram kernels (csrc/gram.hip) add theirs into the same scalar and the same gb."""

    @staticmethod
    def forward(ctx, a, b, c_log, act, gram_w):
        a, b = a.contiguous(), b.contiguous()
        n, ld = b.shape[0], b.shape[-1]
        rows = b.numel() // ld
        hw = rows // n
        partial = torch.empty(L1_BLOCKS, dtype=torch.float32, device=b.device)
        out = torch.empty((), dtype=torch.float32, device=b.device)
        L.call("ups_l1_fwd", L.ptr(a), L.ptr(b), L.dt(b), rows, c_log, ld, act, L.ptr(partial), L1_BLOCKS, L.stream())
        L.call("ups_sum_scale", L.ptr(partial), L1_BLOCKS, 1.0 / (rows * c_log), L.ptr(out), 0, L.stream())
        _, npart, nws, nsign = gram_plan(n, hw, c_log, L.dt(b))
        gpart = torch.empty(npart, dtype=torch.float32, device=b.device)
        sign = torch.empty(nsign, dtype=torch.int8, device=b.device)
        ws = torch.empty(nws, dtype=torch.float32, device=b.device) if nws else None
        L.call("ups_gram_l1_fwd", L.ptr(a), L.ptr(b), L.dt(b), n, hw, c_log, ld, act, L.ptr(gpart), L.ptr(sign), L.ptr(ws),
               L.stream())
        norm = 1.0 / (GRAM_DIV * hw)
        L.call("ups_sum_scale", L.ptr(gpart), npart, gram_w * norm / (n * c_log * c_log), L.ptr(out), 1, L.stream())
        ctx.save_for_backward(a, b, sign)
        ctx.c_log, ctx.act, ctx.gram_w = c_log, act, gram_w
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, sign = ctx.saved_tensors
        n, ld = b.shape[0], b.shape[-1]
        rows = b.numel() // ld
        hw, c_log = rows // n, ctx.c_log
        gb = torch.empty_like(b)
        g = g.contiguous().float()
        L.call("ups_l1_bwd", L.ptr(a), L.ptr(b), L.ptr(gb), L.dt(b), rows, c_log, ld, ctx.act, L.ptr(g),
               1.0 / (rows * c_log), L.stream())
        coef = 2.0 * ctx.gram_w / (n * c_log * c_log) / (GRAM_DIV * hw)
        L.call("ups_gram_l1_bwd", L.ptr(b), L.ptr(sign), L.ptr(gb), L.dt(b), n, hw, c_log, ld, ctx.act, L.ptr(g), coef, L.stream())
        return None, gb, None, None, None


class CriticHeadFn(torch.autograd.Function):
    """Head of a separable MI critic (model.py:159-173 last line, 524-536, 821-826, 855): (h_pi [2B,..,K], h_al [2B,..,K]) ->
    (loss, accuracy, mean joint logit) as three device scalars, rows [0,B) = joint pairs, [B,2B) = marginal pairs.  One launch
    forward, one backward (ups_critic_head_*); the gradient arguments are device scalars -- no host synchronisation."""

    @staticmethod
    def forward(ctx, h_pi, h_al, B, K):
        h_pi, h_al = h_pi.contiguous(), h_al.contiguous()
        ld = h_pi.shape[-1]
        assert h_pi.numel() == 2 * B * ld and h_al.shape == h_pi.shape
        logits = torch.empty(2 * B, dtype=torch.float32, device=h_pi.device)
        out = torch.empty(4, dtype=torch.float32, device=h_pi.device)
        L.call("ups_critic_head_fwd", L.ptr(h_pi), L.ptr(h_al), L.dt(h_pi), B, K, ld, L.ptr(logits), L.ptr(out), L.stream())
        ctx.save_for_backward(h_pi, h_al, logits)
        ctx.B, ctx.K = B, K
        loss, acc, mim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(acc)
        return loss, acc, mim

    @staticmethod
    def backward(ctx, g_loss, g_acc, g_mim):
        h_pi, h_al, logits = ctx.saved_tensors
        ld = h_pi.shape[-1]
        gl = g_loss.contiguous().float() if g_loss is not None else None
        gm = g_mim.contiguous().float() if g_mim is not None else None
        gp = torch.empty_like(h_pi) if ctx.needs_input_grad[0] else None
        ga = torch.empty_like(h_al) if ctx.needs_input_grad[1] else None
        if gp is not None or ga is not None:
            L.call("ups_critic_head_bwd", L.ptr(h_pi), L.ptr(h_al), L.ptr(logits), L.ptr(gl), L.ptr(gm), L.dt(h_pi), ctx.B, ctx.K, ld,
                   L.ptr(gp), L.ptr(ga), L.stream())
        return gp, ga, None, None


TOWERS = SW.flag("UPS_TOWERS")      # A/B switch: the critics' towers as grouped launches (ups_towers_*)


def towers_eligible(towers, xs):
    """towers: [[ConvLayer] * L] * T (nets.Nets.critic_layers), xs: their inputs [M, 1, 1, ld].  The grouped launches take bf16 rows,
    the leaky-ReLU post-activation storage form and widths of 32 k / 128 n; anything else keeps the generic convolution path."""
    if not TOWERS or not towers or len(towers) > 8 or not (2 <= len(towers[0]) <= 6):
        return False
    Ln = len(towers[0])
    for tw, x in zip(towers, xs):
        if len(tw) != Ln or x.dtype != torch.bfloat16 or x.shape[1:3] != (1, 1):
            return False
        for l, lay in enumerate(tw):
            if lay.k != 1 or lay.stride != 1 or lay.coords or lay.f16 or lay.ci_log % 32 or lay.co % 128:
                return False
            want_in = (L.ACT_NONE, False) if l == 0 else (L.ACT_LRELU, True)
            if (lay.act_in, lay.in_post) != want_in or lay.out_act != (L.ACT_LRELU if l < Ln - 1 else L.ACT_NONE):
                return False
            if l > 0 and (lay.ci_log != tw[l - 1].co or (l < Ln - 1 and lay.ci_log != lay.co)):
                return False
        # the checks ups_towers_fwd / _bwd make on the first layer's input (csrc/critic.hip: ld0 >= k, ld0 % 8 == 0, 16-byte aligned
        # rows): a view that fails them keeps the generic path instead of raising UpsError in the middle of a step
        if x.shape[-1] < tw[0].ci_log or x.shape[-1] % 8 or (x.is_contiguous() and x.data_ptr() % 16):
            return False
    for l in range(Ln):                     # one launch per layer index: every tower must have the same width there
        if len(set(tw[l].co for tw in towers)) != 1:
            return False
    return True


class TowersFn(torch.autograd.Function):
    """T towers of nin -> residual_block(k = 1) x (L - 2) -> nin (discriminator_model, model.py:159-173) as grouped launches: the same
    layer of every tower in one launch, every weight / bias gradient in one (ups_towers_fwd / _bwd).  apply(towers, x_0 .. x_{T-1},
    V, b of every layer tower-major) -> the T embeddings [M, 1, 1, n].  A backward call takes the towers whose output gradient it is
    given (the adversarial term differentiates critic 0's pi tower alone, under skip_wgrad)."""

    @staticmethod
    def forward(ctx, towers, *tensors):
        T, Ln = len(towers), len(towers[0])
        xs = [t.contiguous() for t in tensors[:T]]
        M, dev = xs[0].shape[0], xs[0].device
        lay_arr = (L.TowerLayer * (T * Ln))()
        for t, tw in enumerate(towers):
            for l, lay in enumerate(tw):
                ent = lay.prepared(L.BF16, 1, 1)
                e = lay_arr[t * Ln + l]
                e.w_fwd, e.w_dgrad, e.bias = ent["w_fwd"].data_ptr(), ent["w_dgrad"].data_ptr(), lay.b.data_ptr()
                e.grad_w = lay.grad_V.data_ptr() if lay.grad_V is not None else None
                e.grad_b = lay.grad_b.data_ptr() if lay.grad_b is not None else None
                e.k, e.n = lay.ci_log, lay.co
        acts = [[torch.empty((M, 1, 1, lay.co), dtype=torch.bfloat16, device=dev) for lay in tw] for tw in towers]
        x0 = (C.c_void_p * T)(*[x.data_ptr() for x in xs])
        ld0 = (C.c_int32 * T)(*[x.shape[-1] for x in xs])
        ap = (C.c_void_p * (T * Ln))(*[a.data_ptr() for tw in acts for a in tw])
        slope = towers[0][0].slope
        L.call("ups_towers_fwd", lay_arr, T, Ln, x0, ld0, ap, M, slope, L.stream())
        outs = tuple(tw[-1] for tw in acts)
        ctx.save_for_backward(*(xs + list(outs)))            # (the pointer arrays below stay valid while these are alive)
        ctx.inner = [tw[:-1] for tw in acts]
        ctx.towers, ctx.arrays, ctx.M, ctx.slope = towers, (lay_arr, x0, ld0, ap), M, slope
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *gs):
        towers, M = ctx.towers, ctx.M
        T, Ln = len(towers), len(towers[0])
        xs = list(ctx.saved_tensors[:T])
        lay_arr, x0, ld0, ap = ctx.arrays
        dev = xs[0].device
        gout = [None if g is None else to_act_dtype(g, torch.bfloat16, towers[t][-1].co) for t, g in enumerate(gs)]
        want_w = not GradMode.skip_wgrad
        gx = [torch.empty_like(xs[t]) if (gout[t] is not None and ctx.needs_input_grad[1 + t] and towers[t][0].ci_log % 128 == 0
                                          and xs[t].shape[-1] == towers[t][0].ci_log) else None for t in range(T)]
        if any(gout[t] is not None and ctx.needs_input_grad[1 + t] and gx[t] is None for t in range(T)):
            raise L.UpsError("TowersFn: the input gradient of a tower whose first layer is not 128 k wide")
        ws = [[torch.empty((M, lay.co), dtype=torch.bfloat16, device=dev) if (gout[t] is not None and l < Ln - 1) else None
               for l, lay in enumerate(tw)] for t, tw in enumerate(towers)]
        gp = (C.c_void_p * T)(*[None if g is None else g.data_ptr() for g in gout])
        wp = (C.c_void_p * (T * Ln))(*[None if w is None else w.data_ptr() for tw in ws for w in tw])
        gxp = (C.c_void_p * T)(*[None if g is None else g.data_ptr() for g in gx])
        ldg = (C.c_int32 * T)(*[x.shape[-1] for x in xs])
        L.call("ups_towers_bwd", lay_arr, T, Ln, x0, ld0, ap, gp, wp, gxp, ldg, int(want_w), M, ctx.slope, L.stream())
        grads = [None] + gx
        for t, tw in enumerate(towers):
            for lay in tw:
                if want_w and gout[t] is not None and lay.grad_V is not None:
                    grads += [lay.grad_V, lay.grad_b]
                    if lay.after_wgrad is not None:
                        lay.after_wgrad()
                else:
                    grads += [None, None]
        return tuple(grads)


class MaskPartsFn(torch.autograd.Function):
    """mask_parts + part-major transpose (model.py:176-187, nn.py:97-103): -> [P*B,H,W,8]."""

    @staticmethod
    def forward(ctx, view, hard, act_dtype):
        B, H, W, P = hard.shape
        out = torch.empty((P * B, H, W, 8), dtype=act_dtype, device=hard.device)
        L.call("ups_mask_parts_fwd", L.ptr(view), L.ptr(hard), L.ptr(out), L.dt(out), B, H * W, P, L.stream())
        ctx.save_for_backward(view)
        ctx.shape = (B, H, W, P)
        return out

    @staticmethod
    def backward(ctx, g):
        (view,) = ctx.saved_tensors
        B, H, W, P = ctx.shape
        g = g.contiguous()
        gh = torch.empty((B, H, W, P), dtype=torch.float32, device=g.device)
        L.call("ups_mask_parts_bwd", L.ptr(view), L.ptr(g), L.ptr(gh), L.dt(g), B, H * W, P, L.stream())
        return None, gh, None


class UnpoolFn(torch.autograd.Function):
    """unpool_features + concat with the hard mask (model.py:225-249, 482-484): -> [B,H,W,round8(F+P)]."""

    @staticmethod
    def forward(ctx, hard, feat, act_dtype):
        B, H, W, P = hard.shape
        F = feat.shape[-1]
        ldo = round8(F + P)
        feat = feat.contiguous()
        out = torch.empty((B, H, W, ldo), dtype=act_dtype, device=hard.device)
        L.call("ups_unpool_fwd", L.ptr(hard), L.ptr(feat), L.ptr(out), L.dt(out), B, H * W, P, F, ldo, L.stream())
        ctx.save_for_backward(hard, feat)
        return out

    @staticmethod
    def backward(ctx, g):
        hard, feat = ctx.saved_tensors
        B, H, W, P = hard.shape
        F = feat.shape[-1]
        g = g.contiguous()
        gh = torch.empty_like(hard)
        nfl = L.load().ups_unpool_bwd_floats(B, P, F)
        gf = torch.empty(nfl, dtype=torch.float32, device=g.device)
        L.call("ups_unpool_bwd", L.ptr(hard), L.ptr(feat), L.ptr(g), L.ptr(gh), L.ptr(gf), L.dt(g), B, H * W, P, F,
               g.shape[-1], L.stream())
        return gh, gf[:B * P * F].view(B, P, F), None


# --------------------------------------------------------------------------- raw (non-autograd) part-path / latent calls
def part_softmax(mean, eps=None, want_hard=True, want_argmax=False, want_bits=None, moments_gamma=None):
    """-> (l, m, hard, argmax), or (l, m, hard, argmax, hard_bits) when `want_bits` is given (True / False):
    hard_bits [..] int32 = the hard mask as a bit set per pixel (P <= 32; None when not wanted).
    moments_gamma (mean [n,h,w,P]): additionally returns, as the last element, the spatial soft-max moments of
    gamma * hard -- what spatial_moments(hard, gamma) computes -- from the same pass (None when the shape does not allow it)."""
    mean = mean.contiguous()
    pixels, P = mean.numel() // mean.shape[-1], mean.shape[-1]
    l = torch.empty_like(mean) if eps is not None else mean
    m = torch.empty_like(mean)
    hard = torch.empty_like(mean) if want_hard else None
    am = torch.empty(mean.shape[:-1], dtype=torch.int64, device=mean.device) if want_argmax else None
    bits = torch.empty(mean.shape[:-1], dtype=torch.int32, device=mean.device) if want_bits else None
    stats = None
    if moments_gamma is not None and mean.dim() == 4 and P <= 32 and want_hard:
        n, h, w, _ = mean.shape
        # the fused form needs whole pixel tiles that do not straddle two images: the library says what its tile is
        if (h * w) % L.load().ups_part_softmax_moments_tile(P) == 0:
            nint = L.load().ups_part_softmax_moments_ints(pixels, P)
            stats = torch.empty((n, P, 8), dtype=torch.float32, device=mean.device)
            scratch = torch.empty(nint, dtype=torch.int32, device=mean.device)
            L.call("ups_part_softmax_moments_fwd", L.ptr(mean), L.ptr(eps.contiguous()) if eps is not None else None,
                   L.ptr(l) if eps is not None else None, L.ptr(m), L.ptr(hard), L.ptr(am), L.ptr(bits), n, h, w, P,
                   float(moments_gamma), L.ptr(stats), L.ptr(scratch), L.stream())
    if stats is None:
        L.call("ups_part_softmax_fwd", L.ptr(mean), L.ptr(eps.contiguous()) if eps is not None else None,
               L.ptr(l) if eps is not None else None, L.ptr(m), L.ptr(hard), L.ptr(am), L.ptr(bits), pixels, P, L.stream())
    out = (l, m, hard, am) if want_bits is None else (l, m, hard, am, bits)
    return out + (stats,) if moments_gamma is not None else out


def unpool_mix(hard, feat, pose_idx, app_idx, act_dtype):
    """Mixed unpool of appearance transfer (ups_unpool_mix_fwd; inference only, no backward): hard [n,H,W,P] and feat [m,P,F] fp32 on
    the device, pose_idx [K] and app_idx [K,P] integer HOST tensors (or sequences) -> [K,H,W,round8(F+P)] in `act_dtype` with
    out[k] = unpool(hard[pose_idx[k]], rows p of feat[app_idx[k,p]]).  The kernel trusts its indices, so they are checked here, on
    the host values they are uploaded from: an index out of range raises before anything is launched."""
    n, H, W, P = hard.shape
    m, Pf, F = feat.shape
    pi = torch.as_tensor(pose_idx, device="cpu").reshape(-1).to(torch.int64)
    ai = torch.as_tensor(app_idx, device="cpu").reshape(-1).to(torch.int64)
    K = pi.numel()
    if Pf != P or hard.dtype != torch.float32 or feat.dtype != torch.float32:
        raise L.UpsError("unpool_mix: hard [n,H,W,P] and feat [m,P,F] must be fp32 with the same P (got {} {}, {} {})".format(
            tuple(hard.shape), hard.dtype, tuple(feat.shape), feat.dtype))
    if K == 0 or ai.numel() != K * P:
        raise L.UpsError("unpool_mix: pose_idx [K] with K >= 1 and app_idx [K,{}] expected (got {} and {} indices)".format(
            P, K, ai.numel()))
    if int(pi.min()) < 0 or int(pi.max()) >= n or int(ai.min()) < 0 or int(ai.max()) >= m:
        raise L.UpsError("unpool_mix: index out of range: pose_idx in [{}, {}] for {} poses, app_idx in [{}, {}] for {} appearances"
                         .format(int(pi.min()), int(pi.max()), n, int(ai.min()), int(ai.max()), m))
    dev = hard.device
    hard, feat = hard.contiguous(), feat.contiguous()
    pd, ad = pi.to(torch.int32).to(dev), ai.to(torch.int32).to(dev)
    ldo = round8(F + P)
    out = torch.empty((K, H, W, ldo), dtype=act_dtype, device=dev)
    L.call("ups_unpool_mix_fwd", L.ptr(hard), L.ptr(feat), L.ptr(pd), L.ptr(ad), L.ptr(out), L.dt(out),
           K, n, m, H * W, P, F, ldo, L.stream())
    return out


# --------------------------------------------------------------------------- what the evaluation wrappers below share
_LIBRARY_CONSTANTS = {}         # name -> the constants of the library that ``_library_constants`` found equal to Python's


def _given_or_new(fn, name, t, shape, dtype, device, zero=False):
    """The output `name` of wrapper `fn`: a caller's tensor -- contiguous, of `shape` and `dtype` on `device`; a row-offset view of a
    larger buffer is fine -- or None: new zeros (an output the kernel ADDS to) or new empty (one it writes completely).  The counters
    (`invalid`, `changed`, `n_singular`) are [1] int32.  L.UpsError before anything is launched; L.ptr would only assert."""
    if t is None:
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        got = type(t) if not torch.is_tensor(t) else "{} {} on {}{}".format(list(t.shape), t.dtype, t.device,
                                                                               "" if t.is_contiguous() else ", not contiguous")
        raise L.UpsError("{}: {} {} {} contiguous on {} expected (got {})".format(fn, name, list(shape), dtype, device, got))
    return t


def _scratch(nbytes, device):
    """The float64 scratch of a ups_*_scratch_bytes result; a fresh allocation per call (the caching allocator orders its reuse on the
    stream).  0 bytes (sizes the library does not take): one element, and the C entry refuses the call."""
    return torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)


def _library_constants(name, **want):
    """On first use of `name`: every keyword k is a constant of this module that the library exports as ups_<k>() and must agree."""
    if name not in _LIBRARY_CONSTANTS:
        lib = L.load()
        got = {k: getattr(lib, "ups_" + k)() for k in want}
        if got != want:
            raise L.UpsError("the library's {} constants {} differ from ops' {}: rebuild".format(
                name, {k: v for k, v in got.items() if v != want[k]}, {k: v for k, v in want.items() if v != got[k]}))
        _LIBRARY_CONSTANTS[name] = got


# --------------------------------------------------------------------------- part-IoU evaluation (csrc/evalparts.hip)
def part_confusion(pred, gt_u8, P, G, lut=None, counts=None, invalid=None):
    """counts[i,p,g] += #{pixels of image i with pred == p and lut[gt] == g} (ups_part_confusion; the statistic
    evalutil.evaluate_from_counts takes).  pred [N,..] int64 (the arg-max map of part_softmax), gt_u8 [N,..] uint8 of the same shape,
    lut [256] uint8 on the device or None (identity), 1 <= P, G <= 32.  counts [N,P,G] int32 (default: new zeros; given: added to --
    a row-offset view of a larger buffer is fine), invalid [1] int32 (default: new zero): += the pixels with pred outside [0,P) or
    a mapped label >= G, which are counted nowhere else.  Asynchronous on the current stream.  Returns counts."""
    N = pred.shape[0]
    if (pred.dtype != torch.int64 or gt_u8.dtype != torch.uint8 or pred.shape != gt_u8.shape or N == 0
            or (lut is not None and (lut.dtype != torch.uint8 or lut.numel() != 256))):
        raise L.UpsError("part_confusion: pred int64 and gt uint8 of one shape [N >= 1, ..], lut [256] uint8 (got {} {}, {} {}, lut {})"
                         .format(tuple(pred.shape), pred.dtype, tuple(gt_u8.shape), gt_u8.dtype,
                                 None if lut is None else (tuple(lut.shape), lut.dtype)))
    counts = _given_or_new("part_confusion", "counts", counts, (N, P, G), torch.int32, pred.device, zero=True)
    invalid = _given_or_new("part_confusion", "invalid", invalid, (1,), torch.int32, pred.device, zero=True)
    pred, gt_u8 = pred.contiguous(), gt_u8.contiguous()
    L.call("ups_part_confusion", L.ptr(pred), L.ptr(gt_u8), L.ptr(lut), N, pred.numel() // N, P, G, L.ptr(counts), L.ptr(invalid),
           L.stream())
    return counts


# --------------------------------------------------------------------------- label-free validation metrics (csrc/valmetrics.hip)
IMAGE_METRICS_TILE = 32         # valid pixels per tile edge of ups_image_metrics (checked against the library on first use)
PART_USAGE_CHUNK = 1024         # pixels per block of ups_part_usage
SSIM_WINDOW, SSIM_SIGMA = 11, 1.5


def ssim_weights():
    """The 11 normalised float64 weights of the separable SSIM window (Gaussian, sigma 1.5: Wang et al. 2004), as a NumPy array: the
    numbers both the kernel (a host argument) and the host restatement multiply by."""
    import numpy as np
    k = np.arange(SSIM_WINDOW, dtype=np.float64) - SSIM_WINDOW // 2
    w = np.exp(-(k * k) / (2.0 * SSIM_SIGMA * SSIM_SIGMA))
    return w / w.sum()


def _metrics_geometry():
    _library_constants("metrics", image_metrics_tile=IMAGE_METRICS_TILE, part_usage_chunk=PART_USAGE_CHUNK)


def image_metrics(a, b, out=None):
    """out[i] = (sse, sae, ssim_sum) of images a[i], b[i] (ups_image_metrics; the sums evalutil.reconstruction_from_sums takes).
    a, b [N,H,W,>=3] float32 or bfloat16 NHWC, each with its own dtype and channel count (channels 0..2 are read), values in [-1, 1]
    (mapped to [0, 1] and clamped); H, W >= 11.  out [N,3] float64 (default: new; a row-offset view of a larger buffer is fine), written
    completely.  Asynchronous on the current stream; the scratch is a fresh allocation per call (the caching allocator orders its reuse
    on that stream).  Returns out."""
    if (a.dim() != 4 or b.dim() != 4 or tuple(a.shape[:3]) != tuple(b.shape[:3]) or a.shape[0] == 0 or a.shape[3] < 3 or b.shape[3] < 3
            or a.dtype not in _IMG_DTYPES or b.dtype not in _IMG_DTYPES):
        raise L.UpsError("image_metrics: a, b [N >= 1,H,W,>=3] float32 / bfloat16 of one [N,H,W] (got {} {}, {} {})".format(
            tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
    N, H, W = a.shape[:3]
    out = _given_or_new("image_metrics", "out", out, (N, 3), torch.float64, a.device)
    _metrics_geometry()
    a, b = a.contiguous(), b.contiguous()
    scratch = _scratch(L.load().ups_image_metrics_scratch_bytes(N, H, W), a.device)
    w = ssim_weights()
    L.call("ups_image_metrics", L.ptr(a), L.dt(a), a.shape[3], L.ptr(b), L.dt(b), b.shape[3], N, H, W,
           w.ctypes.data_as(C.POINTER(C.c_double)), L.ptr(out), L.ptr(scratch), L.stream())
    return out


def part_usage(soft, pred, counts=None, invalid=None, sharp=None):
    """counts[i,p] += #{pixels of image i with pred == p}; sharp[i] = (sum of max_p soft, sum of -sum_p s ln s) over image i's pixels
    (ups_part_usage; the statistics evalutil.usage_from_counts takes).  soft [N,..,P] float32 (out_parts_soft), pred [N,..] int64
    (out_parts_hard) over the same pixels, P <= 32 (more: L.UpsError from the C entry -- evalutil.PartUsageEvaluator counts on the host
    then).  counts [N,P] int32 (default: new zeros; given: added to), invalid [1] int32 (+= pixels with pred outside [0,P), counted
    nowhere else), sharp [N,2] float64 (written).  Asynchronous on the current stream.  Returns (counts, invalid, sharp)."""
    N, P = pred.shape[0], soft.shape[-1]
    if (soft.dtype != torch.float32 or pred.dtype != torch.int64 or N == 0 or tuple(soft.shape[:-1]) != tuple(pred.shape)):
        raise L.UpsError("part_usage: soft [N >= 1,..,P] float32 and pred [N,..] int64 over the same pixels (got {} {}, {} {})".format(
            tuple(soft.shape), soft.dtype, tuple(pred.shape), pred.dtype))
    counts = _given_or_new("part_usage", "counts", counts, (N, P), torch.int32, pred.device, zero=True)
    invalid = _given_or_new("part_usage", "invalid", invalid, (1,), torch.int32, pred.device, zero=True)
    sharp = _given_or_new("part_usage", "sharp", sharp, (N, 2), torch.float64, pred.device)
    _metrics_geometry()
    soft, pred = soft.contiguous(), pred.contiguous()
    HW = pred.numel() // N
    scratch = _scratch(L.load().ups_part_usage_scratch_bytes(N, HW), pred.device)
    L.call("ups_part_usage", L.ptr(soft), L.ptr(pred), N, HW, P, L.ptr(counts), L.ptr(invalid), L.ptr(sharp), L.ptr(scratch), L.stream())
    return counts, invalid, sharp


# --------------------------------------------------------------------------- part equivariance under TPS warps (csrc/equivariance.hip)
PART_EQUIVARIANCE_CHUNK = 1024  # pixels per block of ups_part_equivariance (checked against the library on first use)


def tps_grid(T, coord, h, w):
    """grid [n,h,w,2] float32 = (px, py): the source pixel position ``ups_tps_warp`` samples for every output pixel of an h x w image
    under T [n,2,K+3], coord [n,K,2] float32 (``tps.tps_system``), in the warp kernel's own fp32 arithmetic (ups_tps_grid).
    Asynchronous on the current stream."""
    if (T.dim() != 3 or coord.dim() != 3 or T.dtype != torch.float32 or coord.dtype != torch.float32 or T.shape[0] == 0
            or coord.shape[0] != T.shape[0] or coord.shape[2] != 2 or tuple(T.shape[1:]) != (2, coord.shape[1] + 3)):
        raise L.UpsError("tps_grid: T [n >= 1,2,K+3] and coord [n,K,2] float32 (got {} {}, {} {})".format(
            tuple(T.shape), T.dtype, tuple(coord.shape), coord.dtype))
    n, K = coord.shape[0], coord.shape[1]
    grid = torch.empty((n, int(h), int(w), 2), dtype=torch.float32, device=T.device)
    L.call("ups_tps_grid", L.ptr(T.contiguous()), L.ptr(coord.contiguous()), L.ptr(grid), n, int(h), int(w), K, L.stream())
    return grid


def part_equivariance(soft_a, soft_b, pred_b, grid, counts=None, invalid=None, tv=None):
    """counts[i,la,lb] += #{inside pixels of image i whose sampled original part is la and whose warped part is lb}; tv[i] = the sum
    of the per-pixel total variation over those pixels (ups_part_equivariance; the definitions: include/upsparts_hip.h; the
    statistics evalutil.equivariance_from_counts takes).  soft_a, soft_b [N,h,w,P] float32 (out_parts_soft of the originals and of
    the warped images), pred_b [N,h,w] int64 (out_parts_hard of the warped images), grid [N,h,w,2] float32 (``tps_grid``), P <= 32
    (more: L.UpsError from the C entry -- evalutil.EquivarianceEvaluator computes on the host then).  counts [N,P,P] int32 (default:
    new zeros; given: added to), invalid [1] int32 (+= inside pixels with a NaN or a pred_b outside [0,P), counted nowhere else),
    tv [N] float64 (written).  Asynchronous on the current stream.  Returns (counts, invalid, tv)."""
    if (soft_a.dim() != 4 or soft_a.dtype != torch.float32 or soft_b.dtype != torch.float32 or pred_b.dtype != torch.int64
            or grid.dtype != torch.float32 or soft_a.shape[0] == 0 or soft_b.shape != soft_a.shape
            or tuple(pred_b.shape) != tuple(soft_a.shape[:3]) or tuple(grid.shape) != tuple(soft_a.shape[:3]) + (2,)):
        raise L.UpsError("part_equivariance: soft_a, soft_b [N >= 1,h,w,P] float32, pred_b [N,h,w] int64 and grid [N,h,w,2] float32 over "
                         "the same pixels (got {} {}, {} {}, {} {}, {} {})".format(
                             tuple(soft_a.shape), soft_a.dtype, tuple(soft_b.shape), soft_b.dtype, tuple(pred_b.shape), pred_b.dtype,
                             tuple(grid.shape), grid.dtype))
    N, h, w, P = soft_a.shape
    dev = soft_a.device
    counts = _given_or_new("part_equivariance", "counts", counts, (N, P, P), torch.int32, dev, zero=True)
    invalid = _given_or_new("part_equivariance", "invalid", invalid, (1,), torch.int32, dev, zero=True)
    tv = _given_or_new("part_equivariance", "tv", tv, (N,), torch.float64, dev)
    _library_constants("equivariance", part_equivariance_chunk=PART_EQUIVARIANCE_CHUNK)
    soft_a, soft_b, pred_b, grid = soft_a.contiguous(), soft_b.contiguous(), pred_b.contiguous(), grid.contiguous()
    scratch = _scratch(L.load().ups_part_equivariance_scratch_bytes(N, h * w), dev)
    L.call("ups_part_equivariance", L.ptr(soft_a), L.ptr(soft_b), L.ptr(pred_b), L.ptr(grid), N, h, w, P, L.ptr(counts), L.ptr(invalid),
           L.ptr(tv), L.ptr(scratch), L.stream())
    return counts, invalid, tv


# --------------------------------------------------------------------------- part-appearance index (csrc/partindex.hip)
PART_KNN_MAX_K, PART_KMEANS_MAX_K = 32, 64


def _bank(what, feat, valid):
    if (feat.dim() != 3 or feat.dtype != torch.float32 or feat.shape[0] == 0 or valid.dtype != torch.uint8
            or tuple(valid.shape) != tuple(feat.shape[:2])):
        raise L.UpsError("{}: codes [N >= 1,P,A] float32 and valid [N,P] uint8 (got {} {}, {} {})".format(
            what, tuple(feat.shape), feat.dtype, tuple(valid.shape), valid.dtype))
    return feat.contiguous(), valid.contiguous()


def part_knn(q, qvalid, g=None, gvalid=None, K=8, exclude_same_index=None):
    """Per part, the K nearest valid gallery codes of every valid query code (ups_part_knn; the definitions: include/upsparts_hip.h,
    restated by tests/partindex_ref.py with equal bits).  q [Nq,P,A] float32 and qvalid [Nq,P] uint8 on the device; g, gvalid: the
    gallery, or None: the query bank itself with self excluded (exclude_same_index then defaults to True, else to False).
    Returns (idx [Nq,P,K] int32, dist [Nq,P,K] float64): ascending in (distance, gallery index), padded with -1 / +inf.  fp64 direct
    squared distances; no distance matrix is written.  Asynchronous on the current stream."""
    if (g is None) != (gvalid is None):
        raise L.UpsError("part_knn: g and gvalid are given together")
    if exclude_same_index is None:
        exclude_same_index = g is None
    q, qvalid = _bank("part_knn", q, qvalid)
    g, gvalid = (q, qvalid) if g is None else _bank("part_knn", g, gvalid)
    if tuple(g.shape[1:]) != tuple(q.shape[1:]) or g.device != q.device:
        raise L.UpsError("part_knn: query {} and gallery {} differ in [P,A] or device".format(tuple(q.shape), tuple(g.shape)))
    Nq, P, A = q.shape
    K = int(K)
    idx = torch.empty((Nq, P, max(K, 0)), dtype=torch.int32, device=q.device)
    dist = torch.empty((Nq, P, max(K, 0)), dtype=torch.float64, device=q.device)
    L.call("ups_part_knn", L.ptr(q), L.ptr(qvalid), Nq, L.ptr(g), L.ptr(gvalid), g.shape[0], P, A, K, int(bool(exclude_same_index)),
           L.ptr(idx), L.ptr(dist), L.stream())
    return idx, dist


def part_kmeans_step(feat, valid, cent, prev_label=None, accumulate=True, changed=None):
    """One k-means step of every part on centroids cent [P,k,A] float64 (ups_part_kmeans_step).  feat [N,P,A] float32, valid [N,P]
    uint8.  Returns a dict: "label" [N,P] int32 (first nearest centroid, -1 where invalid), "mind" [N,P] float64 (+inf where invalid),
    "changed" [1] int32 (+= #{label != prev_label}; given or new zero) and, with accumulate, "counts" [P,k] int32, "sums" [P,k,A]
    float64 (the members' codes added up) and "inertia" [P] float64.  accumulate=False is the assignment alone (the k-means++
    seeding).  The scratch of the per-block partials is a fresh allocation per call (the caching allocator orders its reuse on the
    stream); no floating-point atomics: two calls give the same bits.  Asynchronous on the current stream."""
    feat, valid = _bank("part_kmeans_step", feat, valid)
    N, P, A = feat.shape
    if cent.dim() != 3 or cent.dtype != torch.float64 or cent.shape[0] != P or cent.shape[2] != A or cent.shape[1] == 0:
        raise L.UpsError("part_kmeans_step: cent [{},k >= 1,{}] float64 expected (got {} {})".format(P, A, tuple(cent.shape), cent.dtype))
    if prev_label is not None and (prev_label.dtype != torch.int32 or tuple(prev_label.shape) != (N, P)):
        raise L.UpsError("part_kmeans_step: prev_label [{},{}] int32 expected".format(N, P))
    cent = cent.contiguous()
    k, dev = cent.shape[1], feat.device
    out = {"label": torch.empty((N, P), dtype=torch.int32, device=dev), "mind": torch.empty((N, P), dtype=torch.float64, device=dev),
           "changed": _given_or_new("part_kmeans_step", "changed", changed, (1,), torch.int32, dev, zero=True)}
    scratch = None
    if accumulate:
        out["counts"] = torch.zeros((P, k), dtype=torch.int32, device=dev)
        out["sums"] = torch.empty((P, k, A), dtype=torch.float64, device=dev)
        out["inertia"] = torch.empty((P,), dtype=torch.float64, device=dev)
        scratch = _scratch(L.load().ups_part_kmeans_scratch_bytes(N, P, A, k), dev)
    L.call("ups_part_kmeans_step", L.ptr(feat), L.ptr(valid), N, P, A, L.ptr(cent), k,
           L.ptr(None if prev_label is None else prev_label.contiguous()), L.ptr(out["label"]), L.ptr(out["mind"]),
           L.ptr(out.get("counts")), L.ptr(out.get("sums")), L.ptr(out.get("inertia")), L.ptr(out["changed"]), L.ptr(scratch), L.stream())
    return out


# --------------------------------------------------------------------------- landmark regression evaluation (csrc/landmarks.hip)
PART_MOMENTS_MAX_P, LANDMARK_MAX_D, LANDMARK_MAX_K = 32, 65, 32


def part_moments(soft, pred=None, min_mass=0.0, hard=None, invalid=None):
    """Mass and centre of every part of every image (ups_part_moments; the definitions: include/upsparts_hip.h, restated by
    tests/landmarks_ref.py with equal bits).  soft [N,h,w,P] float32 (out_parts_soft), P <= 32; pred [N,h,w] int64 (out_parts_hard)
    or None.  Returns a dict: "mass" [N,P] float64, "centre" [N,P,2] float64 ((x, y) on [-1, 1]; (0, 0) where not valid), "valid"
    [N,P] uint8 (mass finite, > 0 and >= min_mass) and, with pred, "hard" [N,P,3] int32 (+= count, sum(2x + 1 - w), sum(2y + 1 - h);
    given or new zeros) and "invalid" [1] int32 (+= pixels with pred outside [0,P)).  No floating-point atomics: two calls give the
    same bits.  The scratch is a fresh allocation per call (the caching allocator orders its reuse on the stream).  Asynchronous on the
    current stream."""
    if soft.dim() != 4 or soft.dtype != torch.float32 or soft.shape[0] == 0 or (
            pred is not None and (pred.dtype != torch.int64 or tuple(pred.shape) != tuple(soft.shape[:3]))):
        raise L.UpsError("part_moments: soft [N >= 1,h,w,P] float32 and pred [N,h,w] int64 or None (got {} {}{})".format(
            tuple(soft.shape), soft.dtype, "" if pred is None else ", {} {}".format(tuple(pred.shape), pred.dtype)))
    N, h, w, P = soft.shape
    dev = soft.device
    out = {"mass": torch.empty((N, P), dtype=torch.float64, device=dev), "centre": torch.empty((N, P, 2), dtype=torch.float64, device=dev),
           "valid": torch.empty((N, P), dtype=torch.uint8, device=dev)}
    if pred is not None:
        out["hard"] = _given_or_new("part_moments", "hard", hard, (N, P, 3), torch.int32, dev, zero=True)
        out["invalid"] = _given_or_new("part_moments", "invalid", invalid, (1,), torch.int32, dev, zero=True)
    scratch = _scratch(L.load().ups_part_moments_scratch_bytes(N, h, w, P), dev)
    L.call("ups_part_moments", L.ptr(soft.contiguous()), L.ptr(None if pred is None else pred.contiguous()), N, h, w, P, float(min_mass),
           L.ptr(out["mass"]), L.ptr(out["centre"]), L.ptr(out["valid"]), L.ptr(out.get("hard")), L.ptr(out.get("invalid")),
           L.ptr(scratch), L.stream())
    return out


def _landmark_inputs(what, feat, target, vis):
    if feat.dim() != 2 or feat.dtype != torch.float64 or feat.shape[0] == 0:
        raise L.UpsError("{}: feat [N >= 1,D-1] float64 (got {} {})".format(what, tuple(feat.shape), feat.dtype))
    if target is not None and (target.dim() != 3 or target.dtype != torch.float64 or target.shape[0] != feat.shape[0] or target.shape[2] != 2
                               or target.shape[1] == 0 or vis is None or vis.dtype != torch.uint8
                               or tuple(vis.shape) != tuple(target.shape[:2]) or target.device != feat.device or vis.device != feat.device):
        raise L.UpsError("{}: target [{},K >= 1,2] float64 and vis [N,K] uint8 on feat's device".format(what, feat.shape[0]))


def landmark_gram(feat, target, vis):
    """The normal equations of the per-keypoint linear map (ups_landmark_gram).  feat [N,D-1] float64 (the kernel appends the constant
    1), target [N,K,2] float64, vis [N,K] uint8; D <= 65, K <= 32.  Returns (G [K,D,D], R [K,D,2] float64, cnt [K] int32), sums over
    the items where the keypoint is visible, in the fixed order the header states.  Asynchronous on the current stream."""
    _landmark_inputs("landmark_gram", feat, target, vis)
    N, D, K, dev = feat.shape[0], feat.shape[1] + 1, target.shape[1], feat.device
    G = torch.empty((K, D, D), dtype=torch.float64, device=dev)
    R = torch.empty((K, D, 2), dtype=torch.float64, device=dev)
    cnt = torch.empty((K,), dtype=torch.int32, device=dev)
    scratch = _scratch(L.load().ups_landmark_gram_scratch_bytes(N, D, K), dev)
    L.call("ups_landmark_gram", L.ptr(feat.contiguous()) if D > 1 else None, L.ptr(target.contiguous()), L.ptr(vis.contiguous()), N, D, K,
           L.ptr(G), L.ptr(R), L.ptr(cnt), L.ptr(scratch), L.stream())
    return G, R, cnt


def landmark_solve(G, R, cnt, ridge, n_singular=None):
    """W [K,D,2] float64 with (G_k + ridge diag(1, .., 1, 0)) W_k = R_k by Cholesky (ups_landmark_solve): the bias row is not penalised.
    A keypoint with cnt = 0 or a pivot that is not positive gets W_k = 0 and adds 1 to n_singular ([1] int32 on the device: given, or
    new zero).  Returns (W, n_singular).  Asynchronous on the current stream: nothing is read back here."""
    if (G.dim() != 3 or G.dtype != torch.float64 or G.shape[0] == 0 or G.shape[1] != G.shape[2] or R.dtype != torch.float64
            or tuple(R.shape) != (G.shape[0], G.shape[1], 2) or cnt.dtype != torch.int32 or tuple(cnt.shape) != (G.shape[0],)):
        raise L.UpsError("landmark_solve: G [K,D,D], R [K,D,2] float64 and cnt [K] int32 (got {}, {}, {})".format(
            tuple(G.shape), tuple(R.shape), tuple(cnt.shape)))
    K, D = G.shape[0], G.shape[1]
    n_singular = _given_or_new("landmark_solve", "n_singular", n_singular, (1,), torch.int32, G.device, zero=True)
    W = torch.empty((K, D, 2), dtype=torch.float64, device=G.device)
    L.call("ups_landmark_solve", L.ptr(G.contiguous()), L.ptr(R.contiguous()), L.ptr(cnt.contiguous()), D, K, float(ridge), L.ptr(W),
           L.ptr(n_singular), L.stream())
    return W, n_singular


def landmark_predict(feat, W, target=None, vis=None):
    """pred [N,K,2] = (feat, 1) W_k (ups_landmark_predict) and, with target [N,K,2] float64 and vis [N,K] uint8, d2 [N,K] float64: the
    squared distance where the keypoint is visible, -1 where not.  Returns (pred, d2 or None).  Asynchronous on the current stream."""
    _landmark_inputs("landmark_predict", feat, target, vis)
    N, D = feat.shape[0], feat.shape[1] + 1
    if W.dim() != 3 or W.dtype != torch.float64 or W.shape[0] == 0 or W.shape[1] != D or W.shape[2] != 2 or W.device != feat.device:
        raise L.UpsError("landmark_predict: W [K >= 1,{},2] float64 on feat's device (got {} {})".format(D, tuple(W.shape), W.dtype))
    K = W.shape[0]
    if target is not None and target.shape[1] != K:
        raise L.UpsError("landmark_predict: target [N,{},2] expected (got {})".format(K, tuple(target.shape)))
    pred = torch.empty((N, K, 2), dtype=torch.float64, device=feat.device)
    d2 = None if target is None else torch.empty((N, K), dtype=torch.float64, device=feat.device)
    L.call("ups_landmark_predict", L.ptr(feat.contiguous()) if D > 1 else None, L.ptr(W.contiguous()), N, D, K,
           L.ptr(None if target is None else target.contiguous()), L.ptr(None if vis is None else vis.contiguous()), L.ptr(pred), L.ptr(d2),
           L.stream())
    return pred, d2


# --------------------------------------------------------------------------- segmentation export (csrc/segexport.hip)
SEGMENT_CHUNK = 1024            # pixels per block of ups_segment_render (checked against the library on first use)
SEGMENT_ALIGN = 16              # an image's pixel offset in the packed planes is a multiple of it
SEGMENT_OUTPUTS = ("labels", "overlay", "confidence", "counts")


def segment_table(sizes):
    """sizes [(h, w)] -> (table int32 NumPy [n,4], total): row i = (pixel_offset, h, w, first_block) of image i in the packed planes of
    ups_segment_render.  An image starts where the previous one ends, rounded up to a multiple of 16 pixels (so every image starts
    16-byte aligned in the uint8 planes and a lane stores 4 labels as one dword); first_block is the prefix sum of
    ceil(h * w / SEGMENT_CHUNK); total is the length of a plane in pixels (a multiple of 16).  Host arithmetic only."""
    import numpy as np
    rows, off, blk = [], 0, 0
    for hw in sizes:
        h, w = int(hw[0]), int(hw[1])
        if h < 1 or w < 1:
            raise L.UpsError("segment_table: sizes (h, w) with h, w >= 1 (got {})".format((h, w)))
        rows.append((off, h, w, blk))
        blk += -(-(h * w) // SEGMENT_CHUNK)
        off = -(-(off + h * w) // SEGMENT_ALIGN) * SEGMENT_ALIGN
    if not rows or off > 0x7fffffff or blk > 0x7fffffff:
        raise L.UpsError("segment_table: 1 .. 2^31 - 1 pixels in all (got {} images, {} pixels)".format(len(rows), off))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), off


def segment_pack_sources(sources, table, total):
    """Source images [(h_i, w_i, 3) uint8 NumPy arrays or tensors] -> one pinned uint8 host tensor [total, 3] packed by `table`
    (the alignment gaps are zero)."""
    import numpy as np
    host = torch.zeros((total, 3), dtype=torch.uint8)
    if torch.cuda.is_available():
        host = host.pin_memory()
    flat = host.numpy()
    if len(sources) != len(table):
        raise L.UpsError("segment_render: {} source images for {} sizes".format(len(sources), len(table)))
    for (off, h, w, _), s in zip(table.tolist(), sources):
        a = s.cpu().numpy() if torch.is_tensor(s) else np.asarray(s)
        if a.dtype != np.uint8 or a.shape != (h, w, 3):
            raise L.UpsError("segment_render: a source image of uint8 [{},{},3] expected (got {} {})".format(h, w, a.dtype, a.shape))
        flat[off:off + h * w] = a.reshape(-1, 3)
    return host


SEGMENT_RANGE = 766             # entries of the range table of the guided kernel: L1 distances 0 .. 3 * 255
SEGMENT_MAX_RADIUS = 3


def segment_range_table(sigma):
    """The range weights of the edge-aware refinement: NumPy float64 [766],
    wr[d] = max(exp(-(d/3)^2 / (2 sigma^2)), 2^-64) for the L1 distance d = 0 .. 765 of two RGB bytes triples; sigma > 0 in uint8
    levels of mean absolute channel difference.  The floor keeps every denominator of the kernel positive.  Host arithmetic only."""
    import numpy as np
    sigma = float(sigma)
    if not sigma > 0.0 or sigma == float("inf"):
        raise L.UpsError("segment_range_table: a finite sigma > 0 (got {!r})".format(sigma))
    d = np.arange(SEGMENT_RANGE, dtype=np.float64) / 3.0
    return np.maximum(np.exp(-(d * d) / (2.0 * (sigma * sigma))), 2.0 ** -64)


def _segment_packed_src(src, total):
    if not torch.is_tensor(src) or not src.is_cuda or src.dtype != torch.uint8 or tuple(src.shape) != (total, 3):
        raise L.UpsError("segment_render: packed sources uint8 [{},3] on the device expected (got {})".format(
            total, (tuple(src.shape), src.dtype) if torch.is_tensor(src) else type(src)))
    return src.contiguous()


def segment_guide(src_packed, table, total, S, table_dev=None):
    """The low-resolution photographs the guided kernel compares with: uint8 [n,S,S,3] on the device, guide[i, ty, tx] = the rounded box
    mean of the pixels of image i that tap (ty, tx) covers (ups_segment_guide; integer arithmetic, restated by tests/segrefine_ref.py).
    src_packed: uint8 [total,3] on the device, packed by `table` (segment_table).  Asynchronous on the current stream."""
    import numpy as np
    table = np.ascontiguousarray(table, dtype=np.int32)
    src_packed = _segment_packed_src(src_packed, total)
    if table_dev is None:
        table_dev = torch.from_numpy(table).to(src_packed.device)
    guide = torch.empty((len(table), int(S), int(S), 3), dtype=torch.uint8, device=src_packed.device)
    L.call("ups_segment_guide", L.ptr(src_packed), len(table), int(S), table.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(table_dev),
           total, L.ptr(guide), L.stream())
    return guide


def segment_render(soft, sizes, src=None, colors=None, alpha=0.5, want=("labels",), out=None, refine=None):
    """Label maps / overlays / confidence maps / part counts of n images, image i at its own size sizes[i] = (h, w), in one launch
    (ups_segment_render; the definitions: csrc/segexport.hip, restated by tests/segexport_ref.py with equal bytes).
    soft [n,S,S,P] float32 on the device (out_parts_soft); src: None, a list of uint8 [h_i,w_i,3] images (packed here) or an already
    packed uint8 [total,3] device tensor; colors [P,3] uint8 (device tensor or array; required for the overlay); 0 <= alpha <= 1: the
    colour's weight.  want: any of SEGMENT_OUTPUTS.  out: {name: tensor} of planes to reuse (uint8 [total] / [total,3], counts int32
    [n,P] which is ADDED to); a missing plane is allocated (planes as zeros, so the alignment gaps are defined).
    refine: None, or {"radius": R, "sigma": sigma}: the edge-aware route (needs `src`) -- one ups_segment_guide launch, then
    ups_segment_render_guided with the range table segment_range_table(sigma) in place of ups_segment_render; the guide uint8
    [n,S,S,3] is returned as "guide".
    Returns {"table" (NumPy), "table_dev", "total", <the wanted packed tensors>, "views": {name: [per-image views [h,w] / [h,w,3]]}}.
    Asynchronous on the current stream."""
    _library_constants("segment", segment_chunk=SEGMENT_CHUNK, segment_table_words=4)
    want = tuple(want)
    if not want or any(k not in SEGMENT_OUTPUTS for k in want):
        raise L.UpsError("segment_render: want is a non-empty subset of {} (got {})".format(SEGMENT_OUTPUTS, want))
    if not torch.is_tensor(soft) or not soft.is_cuda or soft.dim() != 4 or soft.dtype != torch.float32 or soft.shape[1] != soft.shape[2]:
        raise L.UpsError("segment_render: soft [n,S,S,P] float32 on the device expected (got {})".format(
            (tuple(soft.shape), soft.dtype) if torch.is_tensor(soft) else type(soft)))
    n, S, _, P = soft.shape
    if len(sizes) != n:
        raise L.UpsError("segment_render: {} sizes for {} maps".format(len(sizes), n))
    if refine is not None:
        if not isinstance(refine, dict) or set(refine) != {"radius", "sigma"}:
            raise L.UpsError("segment_render: refine is None or {{'radius': R, 'sigma': sigma}} (got {!r})".format(refine))
        radius = refine["radius"]
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= SEGMENT_MAX_RADIUS:
            raise L.UpsError("segment_render: refine radius is an integer in 0 .. {} (got {!r})".format(SEGMENT_MAX_RADIUS, radius))
        range_w = segment_range_table(refine["sigma"])
        if src is None:
            raise L.UpsError("segment_render: refine compares with the source images: `src` is required")
    dev = soft.device
    table, total = segment_table(sizes)
    table_dev = torch.from_numpy(table).to(dev)
    soft = soft.contiguous()
    if "overlay" in want and colors is None:
        raise L.UpsError("segment_render: the overlay needs `colors` [P,3] uint8")
    if colors is not None:
        colors = torch.as_tensor(colors).to(dev).contiguous()
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (P, 3):
            raise L.UpsError("segment_render: colors [{},3] uint8 expected (got {} {})".format(P, tuple(colors.shape), colors.dtype))
    if src is not None and not torch.is_tensor(src):
        src = segment_pack_sources(src, table, total).to(dev, non_blocking=True)
    if src is not None and (not src.is_cuda or src.dtype != torch.uint8 or tuple(src.shape) != (total, 3)):
        raise L.UpsError("segment_render: packed sources uint8 [{},3] on the device expected (got {} {})".format(
            total, tuple(src.shape), src.dtype))
    shapes = {"labels": ((total,), torch.uint8), "overlay": ((total, 3), torch.uint8), "confidence": ((total,), torch.uint8),
              "counts": ((n, P), torch.int32)}
    res = {"table": table, "table_dev": table_dev, "total": total}
    for k in want:
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.zeros(shapes[k][0], dtype=shapes[k][1], device=dev)
        if not t.is_cuda or t.dtype != shapes[k][1] or tuple(t.shape) != shapes[k][0] or not t.is_contiguous():
            raise L.UpsError("segment_render: out[{!r}] {} {} expected (got {} {})".format(k, shapes[k][1], shapes[k][0], t.dtype,
                                                                                         tuple(t.shape)))
        res[k] = t
    if refine is not None:
        src = _segment_packed_src(src, total)
        res["guide"] = segment_guide(src, table, total, S, table_dev)
        L.call("ups_segment_render_guided", L.ptr(soft), n, S, P, table.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(table_dev), total,
               L.ptr(src), L.ptr(res["guide"]), L.ptr(torch.from_numpy(range_w).to(dev)), radius, L.ptr(colors), float(alpha),
               L.ptr(res.get("labels")), L.ptr(res.get("overlay")), L.ptr(res.get("confidence")), L.ptr(res.get("counts")), L.stream())
        res["views"] = {k: segment_views(res[k], table) for k in want if k != "counts"}
        return res
    L.call("ups_segment_render", L.ptr(soft), n, S, P, table.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(table_dev), total,
           L.ptr(src.contiguous()) if src is not None else None, L.ptr(colors), float(alpha), L.ptr(res.get("labels")),
           L.ptr(res.get("overlay")), L.ptr(res.get("confidence")), L.ptr(res.get("counts")), L.stream())
    res["views"] = {k: segment_views(res[k], table) for k in want if k != "counts"}
    return res


def segment_views(plane, table):
    """The per-image views [h,w] (or [h,w,3]) of a packed plane [total] (or [total,3]), device or host, by `table`."""
    tail = tuple(plane.shape[1:])
    return [plane[off:off + h * w].view((h, w) + tail) for off, h, w, _ in table.tolist()]


# --------------------------------------------------------------------------- part coherence (csrc/components.hip)
COMPONENTS_TILE = 32            # tile edge of the LDS stage of ups_label_components (checked against the library on first use)
COMPONENTS_MAX_HW = 1 << 20     # pixels per image
COMPONENTS_MAX_P = 255
_COMPONENTS_TABLES = {}         # (N, h, w, device) -> the table of a regular batch, host and device: built once, no copy per call


class _ComponentsLayout(object):
    """Where the images of one call lie: the packed planes' table (host, device), total, n, and whether the caller's tensors are
    a regular [N,h,w] batch (`batch`: (N, h, w); its row stride in the plane is h * w rounded up to SEGMENT_ALIGN) or packed planes."""

    def __init__(self, fn, labels, sizes, table):
        import numpy as np
        self.fn = fn
        if not torch.is_tensor(labels) or not labels.is_cuda or labels.dtype not in (torch.uint8, torch.int64) or labels.numel() == 0:
            raise L.UpsError("{}: labels uint8 or int64 on the device expected (got {})".format(
                fn, (tuple(labels.shape), labels.dtype, labels.device) if torch.is_tensor(labels) else type(labels)))
        self.device = labels.device
        self.label_dtype = labels.dtype
        if sizes is None and table is None:
            if labels.dim() != 3:
                raise L.UpsError("{}: a regular batch is [N,h,w]; packed planes need `sizes` (got {})".format(fn, tuple(labels.shape)))
            N, h, w = (int(v) for v in labels.shape)
            key = (N, h, w, self.device)
            if key not in _COMPONENTS_TABLES:
                tab, total = segment_table([(h, w)] * N)
                _COMPONENTS_TABLES[key] = (tab, torch.from_numpy(tab).to(self.device), total)
            self.table, self.table_dev, self.total = _COMPONENTS_TABLES[key]
            self.batch, self.stride = (N, h, w), -(-(h * w) // SEGMENT_ALIGN) * SEGMENT_ALIGN
        else:
            if table is not None:
                self.table, self.table_dev, self.total = table
                self.table = np.ascontiguousarray(self.table, dtype=np.int32)
            else:
                self.table, self.total = segment_table(sizes)
                self.table_dev = torch.from_numpy(self.table).to(self.device)
            self.batch = None
        self.n = len(self.table)
        hw = self.table[:, 1].astype(np.int64) * self.table[:, 2]
        if int(hw.max()) > COMPONENTS_MAX_HW:
            raise L.UpsError("{}: at most 2^20 pixels per image (got {})".format(fn, int(hw.max())))

    def plane(self, name, t, dtype):
        """The packed plane [total] of a caller's input `name`: itself when it is one (or a regular batch without padding), else a
        packed copy of the regular batch."""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != dtype:
            raise L.UpsError("{}: {} {} on {} expected (got {})".format(
                self.fn, name, dtype, self.device, (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t)))
        if self.batch is None:
            if tuple(t.shape) != (self.total,):
                raise L.UpsError("{}: {} is a packed plane [{}] (got {})".format(self.fn, name, self.total, tuple(t.shape)))
            return t.contiguous()
        N, h, w = self.batch
        if tuple(t.shape) != (N, h, w):
            raise L.UpsError("{}: {} [{},{},{}] expected (got {})".format(self.fn, name, N, h, w, tuple(t.shape)))
        if self.stride == h * w:
            return t.contiguous().view(-1)
        p = torch.zeros(self.total, dtype=dtype, device=self.device)
        p.view(N, self.stride)[:, :h * w] = t.reshape(N, h * w)
        return p

    def out_plane(self, name, t, dtype, tail=()):
        """A packed output plane: the caller's [total] + tail tensor, or new zeros (so that the gaps are defined)."""
        return _given_or_new(self.fn, name, t, (self.total,) + tuple(tail), dtype, self.device, zero=True)

    def shaped(self, p):
        """A packed plane in the caller's form: [N,h,w] (a strided view when h * w is no multiple of 16) for a regular batch."""
        if self.batch is None:
            return p
        N, h, w = self.batch
        return p.view(N, self.stride)[:, :h * w].reshape(N, h, w) if self.stride != h * w else p.view(N, h, w)

    def args(self):
        return self.n, self.table.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(self.table_dev), self.total


def _components_P(fn, P):
    if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= COMPONENTS_MAX_P:
        raise L.UpsError("{}: P is an integer in 1 .. {} (got {!r})".format(fn, COMPONENTS_MAX_P, P))
    _library_constants("components", components_tile=COMPONENTS_TILE)


def components_check(err):
    """Raise L.UpsError if the error flag of label_components is set (a label-chasing loop of the kernels reached its bound: a bug in
    them, never a property of the map).  Reads one int32: synchronises with the stream that ran the kernels."""
    v = int(err.reshape(-1)[0].item())
    if v != 0:
        raise L.UpsError("label_components: a bounded device loop reached its bound (flag {}): the component map is not valid".format(v))


def label_components(labels, P, conn=8, sizes=None, comp=None, err=None, table=None):
    """comp = the connected components of integer label maps (ups_label_components; the definitions: include/upsparts_hip.h "part
    coherence", restated by tests/components_ref.py): comp[k] int32 = the smallest in-image index y * w + x of the component of pixel
    k, -1 where the label is outside [0, P).  labels: uint8 or int64 on the device -- a regular batch [N,h,w] (sizes=None), or a
    packed plane [total] of images of sizes [(h_i, w_i)] laid out by segment_table(sizes) (or table=(table, table_dev, total) of a
    segment_render result).  conn: 4 or 8.  comp: a packed int32 plane [total] to reuse, default new.  err [1] int32 (default: new
    zero): |= 1 if a device loop reached its bound; components_check(err) raises on it.  Asynchronous on the current stream.
    Returns (comp in the form of labels, err)."""
    fn = "label_components"
    _components_P(fn, P)
    if conn not in (4, 8):
        raise L.UpsError("{}: conn is 4 or 8 (got {!r})".format(fn, conn))
    lay = _ComponentsLayout(fn, labels, sizes, table)
    lab = lay.plane("labels", labels, lay.label_dtype)
    comp = lay.out_plane("comp", comp, torch.int32)
    err = _given_or_new(fn, "err", err, (1,), torch.int32, lay.device, zero=True)
    scratch = _scratch(L.load().ups_label_components_scratch_bytes(lay.total), lay.device)
    n, th, td, total = lay.args()
    L.call("ups_label_components", L.ptr(lab), lab.element_size(), n, th, td, total, P, conn, L.ptr(comp), L.ptr(err), L.ptr(scratch),
           L.stream())
    return lay.shaped(comp), err


def label_component_stats(labels, comp, P, small=0, sizes=None, area=None, stats=None, invalid=None, table=None):
    """Component sizes and per-part statistics (ups_label_component_stats).  labels, sizes, table as for label_components; comp: its
    result for the same labels.  area int32 (packed plane to reuse, default new): the pixel count of the pixel's component, 0 where
    invalid.  stats [n,P,4] int32 (default: new zeros; given: ADDED to): pixels, components, largest component (a maximum), components
    with area < small.  invalid [1] int32 += the invalid pixels.  Asynchronous on the current stream.
    Returns (area in the form of labels, stats, invalid)."""
    fn = "label_component_stats"
    _components_P(fn, P)
    if isinstance(small, bool) or not isinstance(small, int) or small < 0:
        raise L.UpsError("{}: small is an integer >= 0 (got {!r})".format(fn, small))
    lay = _ComponentsLayout(fn, labels, sizes, table)
    lab = lay.plane("labels", labels, lay.label_dtype)
    comp = lay.plane("comp", comp, torch.int32)
    area = lay.out_plane("area", area, torch.int32)
    stats = _given_or_new(fn, "stats", stats, (lay.n, P, 4), torch.int32, lay.device, zero=True)
    invalid = _given_or_new(fn, "invalid", invalid, (1,), torch.int32, lay.device, zero=True)
    scratch = _scratch(L.load().ups_label_component_stats_scratch_bytes(lay.total), lay.device)
    n, th, td, total = lay.args()
    L.call("ups_label_component_stats", L.ptr(lab), lab.element_size(), L.ptr(comp), n, th, td, total, P, min(small, 0x7fffffff),
           L.ptr(area), L.ptr(stats), L.ptr(invalid), L.ptr(scratch), L.stream())
    return lay.shaped(area), stats, invalid


def label_components_clean(labels, comp, area, P, min_area, sizes=None, out=None, changed=None, src=None, colors=None, alpha=0.5,
                           overlay=None, confidence=None, counts=None, table=None):
    """One round of speck clean-up (ups_label_components_clean): every component with area < min_area takes the first label of maximal
    vote among its pixels' four edge neighbours that lie in components that are not small; without such a neighbour it stays.
    labels, sizes, table as for label_components; comp, area: the results of label_components / label_component_stats for the same
    labels.  out: a packed plane of labels' dtype (default new; `labels` itself is allowed for a packed plane); changed [1] int32 += the
    relabelled pixels.  Optional planes of a segment_render result, updated at the relabelled pixels only: overlay uint8 [total,3]
    (blended anew from src uint8 [total,3] with `colors` [P,3] and alpha, as segment_render does), confidence uint8 [total] (= 0),
    counts int32 [n,P] (the old part -= 1, the new += 1).  Asynchronous on the current stream.
    Returns (out in the form of labels, changed)."""
    fn = "label_components_clean"
    _components_P(fn, P)
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 1:
        raise L.UpsError("{}: min_area is an integer >= 1 (got {!r})".format(fn, min_area))
    if not 0.0 <= float(alpha) <= 1.0:
        raise L.UpsError("{}: 0 <= alpha <= 1 (got {!r})".format(fn, alpha))
    lay = _ComponentsLayout(fn, labels, sizes, table)
    lab = lay.plane("labels", labels, lay.label_dtype)
    comp = lay.plane("comp", comp, torch.int32)
    area = lay.plane("area", area, torch.int32)
    out = lay.out_plane("out", out, lay.label_dtype)
    changed = _given_or_new(fn, "changed", changed, (1,), torch.int32, lay.device, zero=True)
    if overlay is not None and colors is None:
        raise L.UpsError("{}: the overlay needs `colors` [P,3] uint8".format(fn))
    if colors is not None:
        colors = torch.as_tensor(colors).to(lay.device).contiguous()
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (P, 3):
            raise L.UpsError("{}: colors [{},3] uint8 expected (got {} {})".format(fn, P, tuple(colors.shape), colors.dtype))
    if src is not None:
        src = _given_or_new(fn, "src", src, (lay.total, 3), torch.uint8, lay.device)
    if overlay is not None:
        overlay = _given_or_new(fn, "overlay", overlay, (lay.total, 3), torch.uint8, lay.device)
    if confidence is not None:
        confidence = _given_or_new(fn, "confidence", confidence, (lay.total,), torch.uint8, lay.device)
    if counts is not None:
        counts = _given_or_new(fn, "counts", counts, (lay.n, P), torch.int32, lay.device)
    scratch = _scratch(L.load().ups_label_components_clean_scratch_bytes(lay.total), lay.device)
    n, th, td, total = lay.args()
    L.call("ups_label_components_clean", L.ptr(lab), lab.element_size(), L.ptr(comp), L.ptr(area), n, th, td, total, P,
           min(min_area, 0x7fffffff), L.ptr(out), L.ptr(changed), L.ptr(src), L.ptr(colors), float(alpha), L.ptr(overlay),
           L.ptr(confidence), L.ptr(counts), L.ptr(scratch), L.stream())
    return lay.shaped(out), changed


# --------------------------------------------------------------------------- run-length annotations (csrc/segrle.hip)
SEGMENT_RLE_CHUNK = 1024        # positions k of one chunk of ups_segment_rle_* (checked against the library on first use)


def segment_rle(labels, P, sizes=None, table=None):
    """COCO run-length encoding of every (image, part) mask of a label plane (ups_segment_rle_count, one read of the total, then
    ups_segment_rle_write; the definitions: include/upsparts_hip.h "run-length annotations", restated by tests/segrle_ref.py).
    labels: uint8 on the device -- the packed plane [total] of a ``segment_render`` result with table=(table, table_dev, total) (or
    `sizes`, laid out by segment_table), or a regular batch [N,h,w].  A label >= P belongs to no part.
    Returns {"offsets" int64 [n P + 1], "counts" int32 [offsets[n P]], "area" int32 [n,P], "bbox" int32 [n,P,4] (x, y, w, h)} on the
    device: list (i, p) is counts[offsets[i P + p] : offsets[i P + p + 1]], uncompressed counts in column-major order.  Reads one
    int64 between the two launches (it sizes `counts`): synchronises with the current stream."""
    fn = "segment_rle"
    if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= COMPONENTS_MAX_P:
        raise L.UpsError("{}: P is an integer in 1 .. {} (got {!r})".format(fn, COMPONENTS_MAX_P, P))
    _library_constants("segment_rle", segment_rle_chunk=SEGMENT_RLE_CHUNK)
    lay = _ComponentsLayout(fn, labels, sizes, table)
    lab = lay.plane("labels", labels, torch.uint8)
    n, th, td, total = lay.args()
    dev = lay.device
    offsets = torch.empty(n * P + 1, dtype=torch.int64, device=dev)
    area = torch.empty((n, P), dtype=torch.int32, device=dev)
    bbox = torch.empty((n, P, 4), dtype=torch.int32, device=dev)
    scratch = _scratch(L.load().ups_segment_rle_scratch_bytes(n, total, P), dev)
    L.call("ups_segment_rle_count", L.ptr(lab), n, th, td, total, P, L.ptr(offsets), L.ptr(area), L.ptr(bbox), L.ptr(scratch),
           L.stream())
    n_counts = int(offsets[n * P].item())               # the one read: it sizes the lists
    counts = torch.empty(n_counts, dtype=torch.int32, device=dev)
    L.call("ups_segment_rle_write", L.ptr(lab), n, th, td, total, P, L.ptr(offsets), L.ptr(scratch), L.ptr(counts), n_counts, n_counts,
           L.stream())
    return {"offsets": offsets, "counts": counts, "area": area, "bbox": bbox}


def rle_lists(offsets, counts, n, P):
    """Host copies of segment_rle's offsets and counts (tensors or arrays) -> [[counts of (i, p) as a list of int] * P] * n."""
    import numpy as np
    off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
    cnt = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts).reshape(-1)
    if off.size != n * P + 1 or off[0] != 0 or np.any(np.diff(off) < 1) or off[-1] != cnt.size:
        raise L.UpsError("rle_lists: offsets [{}] ascending from 0 to len(counts) = {} expected (got [{}], {} .. {})".format(
            n * P + 1, cnt.size, off.size, off[0] if off.size else None, off[-1] if off.size else None))
    flat = cnt.tolist()
    o = off.tolist()
    return [[flat[o[i * P + p]:o[i * P + p + 1]] for p in range(P)] for i in range(n)]


# --------------------------------------------------------------------------- training image logs (csrc/canvas.hip): uint8 canvases
def canvas_grid(n, cols=None):
    """(rows, cols) of tf_batch_to_canvas for n tiles (re-derived, UNVERIFIED): cols=None -> the square grid of side ceil(sqrt(n)),
    else ceil(n / cols) rows."""
    n = int(n)
    if n < 1 or (cols is not None and int(cols) < 1):
        raise L.UpsError("canvas_grid: n >= 1 tiles in cols >= 1 columns (got {} in {})".format(n, cols))
    if cols is None:
        g = L.load().ups_canvas_grid_side(n)
        return g, g
    return -(-n // int(cols)), int(cols)


def _canvas_src(what, t, ndim, dtypes, last=None):
    """The sources the canvas kernels take: device, contiguous (the channel stride is the last extent), of one of `dtypes`."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != ndim or t.dtype not in dtypes or not t.is_contiguous() or t.numel() == 0 \
            or (last is not None and t.shape[-1] < last):
        raise L.UpsError("{}: a contiguous {}-D device tensor of {}{} expected (got {})".format(
            what, ndim, " / ".join(str(d) for d in dtypes), "" if last is None else " with >= {} channels".format(last),
            "{} {} contiguous={}".format(tuple(t.shape), t.dtype, t.is_contiguous()) if torch.is_tensor(t) else type(t).__name__))
    return t


def _canvas_out(what, out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_cuda or not out.is_contiguous() or out.data_ptr() % 16:
        raise L.UpsError("{}: out must be a contiguous 16-byte aligned uint8 device tensor {} (got {} {})".format(
            what, tuple(shape), tuple(out.shape), out.dtype))
    return out


_IMG_DTYPES = (torch.float32, torch.bfloat16)


def canvas_images(x, cols=None, out=None):
    """x [N,H,W,ld >= 3] fp32 / bf16 in [-1,1] (channels 0..2 are R, G, B; `generated` comes with 8) -> uint8 [rows*H, cols*W, 3]
    (ups_canvas_images).  Bytes: uint8(clamp((v + 1) * 127.5, 0, 255)), truncating; missing tiles 127."""
    x = _canvas_src("canvas_images: x [N,H,W,ld]", x, 4, _IMG_DTYPES, last=3)
    N, H, W, ld = x.shape
    rows, cols = canvas_grid(N, cols)
    out = _canvas_out("canvas_images", out, (rows * H, cols * W, 3), x.device)
    L.call("ups_canvas_images", L.ptr(x), L.dt(x), N, H, W, ld, rows, cols, L.ptr(out), L.stream())
    return out


def canvas_mask_rgb(colors, mask=None, bits=None, n_parts=None, one_hot=False, cols=None, out=None):
    """mask2rgb as a canvas (ups_canvas_mask_rgb): colors uint8 [P,3] on the device (quantised by the host); exactly one of
    mask [N,H,W,P] fp32 (arg-max, lowest index on ties; one_hot=True: taken as one-hot already, nn.mask2rgb(make_hot=False)) and
    bits [N,H,W] int32 (the hard bits of part_softmax, n_parts <= 32) -> uint8 [rows*H, cols*W, 3]."""
    if (mask is None) == (bits is None):
        raise L.UpsError("canvas_mask_rgb: exactly one of mask and bits")
    if mask is not None:
        mask = _canvas_src("canvas_mask_rgb: mask [N,H,W,P]", mask, 4, (torch.float32,))
        N, H, W, P = mask.shape
    else:
        bits = _canvas_src("canvas_mask_rgb: bits [N,H,W]", bits, 3, (torch.int32,))
        N, H, W = bits.shape
        P = int(n_parts or 0)
        if not 1 <= P <= 32:
            raise L.UpsError("canvas_mask_rgb: bits need 1 <= n_parts <= 32 (got {})".format(n_parts))
    colors = _canvas_src("canvas_mask_rgb: colors [P,3]", colors, 2, (torch.uint8,))
    if tuple(colors.shape) != (P, 3):
        raise L.UpsError("canvas_mask_rgb: colors must be uint8 [{},3] (got {})".format(P, tuple(colors.shape)))
    rows, cols = canvas_grid(N, cols)
    src = mask if mask is not None else bits
    out = _canvas_out("canvas_mask_rgb", out, (rows * H, cols * W, 3), src.device)
    L.call("ups_canvas_mask_rgb", L.ptr(mask), L.ptr(bits), int(bool(one_hot)), L.ptr(colors), N, H, W, P, rows, cols, L.ptr(out),
           L.stream())
    return out


def canvas_assigned_parts(view0, view1, hard0=None, hard1=None, bits0=None, bits1=None, n_parts=None, out=None):
    """assigned_parts (model.py:990-1006) in one launch (ups_canvas_assigned_parts): views [B,H,W,ld >= 3] fp32 / bf16 (same dtype
    and shape), the hard masks of view 0 and view 1 as hard0 / hard1 [B,H,W,P] fp32 or bits0 / bits1 [B,H,W] int32 (n_parts <= 32)
    -> uint8 [ceil(P/5)*g*H, 5*g*W, 3], g = ceil(sqrt(2B))."""
    view0 = _canvas_src("canvas_assigned_parts: view0 [B,H,W,ld]", view0, 4, _IMG_DTYPES, last=3)
    view1 = _canvas_src("canvas_assigned_parts: view1 [B,H,W,ld]", view1, 4, _IMG_DTYPES, last=3)
    if view0.shape != view1.shape or view0.dtype != view1.dtype:
        raise L.UpsError("canvas_assigned_parts: the two views must agree in shape and dtype (got {} {}, {} {})".format(
            tuple(view0.shape), view0.dtype, tuple(view1.shape), view1.dtype))
    B, H, W, ld = view0.shape
    by_bits = bits0 is not None
    if by_bits == (hard0 is not None) or (bits1 is None) != (bits0 is None) or (hard1 is None) != (hard0 is None):
        raise L.UpsError("canvas_assigned_parts: either hard0 and hard1 or bits0 and bits1")
    if by_bits:
        P = int(n_parts or 0)
        if not 1 <= P <= 32:
            raise L.UpsError("canvas_assigned_parts: bits need 1 <= n_parts <= 32 (got {})".format(n_parts))
        for nm, b in (("bits0", bits0), ("bits1", bits1)):
            if tuple(_canvas_src("canvas_assigned_parts: " + nm + " [B,H,W]", b, 3, (torch.int32,)).shape) != (B, H, W):
                raise L.UpsError("canvas_assigned_parts: {} must be [{},{},{}] (got {})".format(nm, B, H, W, tuple(b.shape)))
    else:
        P = hard0.shape[-1] if torch.is_tensor(hard0) and hard0.dim() == 4 else 0
        for nm, h in (("hard0", hard0), ("hard1", hard1)):
            if tuple(_canvas_src("canvas_assigned_parts: " + nm + " [B,H,W,P]", h, 4, (torch.float32,)).shape) != (B, H, W, P):
                raise L.UpsError("canvas_assigned_parts: {} must be [{},{},{},{}] (got {})".format(nm, B, H, W, P, tuple(h.shape)))
    g = canvas_grid(2 * B)[0]
    out = _canvas_out("canvas_assigned_parts", out, (-(-P // 5) * g * H, 5 * g * W, 3), view0.device)
    L.call("ups_canvas_assigned_parts", L.ptr(hard0), L.ptr(hard1), L.ptr(bits0), L.ptr(bits1), L.ptr(view0), L.ptr(view1), L.dt(view0),
           ld, B, H, W, P, L.ptr(out), L.stream())
    return out


CANVAS_LEVELS = (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9)        # model.py:1009
CANVAS_RATIOS = (1.0e-3, 5 * 1.0e-3, 1.0e-2, 5 * 1.0e-2)       # model.py:1021


def canvas_first_item(m, table, hard=None, bits=None, levels=CANVAS_LEVELS, ratios=CANVAS_RATIOS, out=None):
    """The four canvases of batch item 0 in one launch (ups_canvas_first_item): m [H,W,P] fp32 (m0_sample[0]), its hard mask as
    hard [H,W,P] fp32 or bits [H,W] int32 (P <= 32), table uint8 [256,3] on the device (viridis, quantised by the host) ->
    (levels [P*H, 7*W, 1], edges [P*H, 4*W, 1], p_heatmap [g*H, g*W, 3], masks [g*H, g*W, 1]), g = ceil(sqrt(P)).  The maps are in
    [0,1] and go through the quantisation of every other image: gray (127) to white (255)."""
    m = _canvas_src("canvas_first_item: m [H,W,P]", m, 3, (torch.float32,))
    H, W, P = m.shape
    if (hard is None) == (bits is None):
        raise L.UpsError("canvas_first_item: exactly one of hard and bits")
    if hard is not None:
        if tuple(_canvas_src("canvas_first_item: hard [H,W,P]", hard, 3, (torch.float32,)).shape) != (H, W, P):
            raise L.UpsError("canvas_first_item: hard must be [{},{},{}] (got {})".format(H, W, P, tuple(hard.shape)))
    else:
        if tuple(_canvas_src("canvas_first_item: bits [H,W]", bits, 2, (torch.int32,)).shape) != (H, W) or P > 32:
            raise L.UpsError("canvas_first_item: bits must be [{},{}] with P <= 32 (got {}, P = {})".format(H, W, tuple(bits.shape), P))
    table = _canvas_src("canvas_first_item: table [256,3]", table, 2, (torch.uint8,))
    if tuple(table.shape) != (256, 3):
        raise L.UpsError("canvas_first_item: table must be uint8 [256,3] (got {})".format(tuple(table.shape)))
    nl, nr = len(levels), len(ratios)
    if not (1 <= nl <= 8 and 1 <= nr <= 8):
        raise L.UpsError("canvas_first_item: 1..8 levels and 1..8 ratios (got {} and {})".format(nl, nr))
    g = canvas_grid(P)[0]
    shapes = ((P * H, nl * W, 1), (P * H, nr * W, 1), (g * H, g * W, 3), (g * H, g * W, 1))
    out = [None] * 4 if out is None else list(out)
    out = [_canvas_out("canvas_first_item", o, sh, m.device) for o, sh in zip(out, shapes)]
    L.call("ups_canvas_first_item", L.ptr(m), L.ptr(hard), L.ptr(bits), H, W, P, (C.c_float * nl)(*levels), nl, (C.c_float * nr)(*ratios), nr,
           L.ptr(table), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), L.stream())
    return tuple(out)


def spatial_moments(x, gamma, rect_px=None, half=0, kl_sums=None):
    """kl_sums (fp32 [>= 16] device buffer): the same pass also writes sum x * log(P x + 1e-20) -- the categorical KL of the map,
    view 1's other prior term -- to kl_sums[0] (ups_spatial_moments_kl)."""
    n, h, w, P = x.shape
    nfl = L.load().ups_spatial_moments_floats(n, P)
    buf = torch.empty(nfl, dtype=torch.float32, device=x.device)
    if kl_sums is not None:
        L.call("ups_spatial_moments_kl", L.ptr(x), n, h, w, P, float(gamma), L.ptr(rect_px), half, half, L.ptr(buf), L.ptr(kl_sums),
               L.stream())
    else:
        L.call("ups_spatial_moments", L.ptr(x), n, h, w, P, float(gamma), L.ptr(rect_px), half, half, L.ptr(buf), L.stream())
    return buf[:n * P * 8].view(n, P, 8)


def moments_to_px(stats, h, order="xy"):
    """(row, column) centres of the rectangles; order "xy": tfutils.draw_rect reads the (y, x) pair as (x, y)."""
    n, P, _ = stats.shape
    px = torch.empty((n, P, 2), dtype=torch.int32, device=stats.device)
    L.call("ups_moments_to_px", L.ptr(stats), n * P, h, int(order == "xy"), L.ptr(px), L.stream())
    return px


def draw_rect(px, h, w, half):
    n, P, _ = px.shape
    out = torch.empty((n, h, w, P), dtype=torch.float32, device=px.device)
    L.call("ups_draw_rect", L.ptr(px), n, h, w, P, half, half, L.ptr(out), L.stream())
    return out


def latent_fwd(params, eps, levels, want_kl):
    """params [B,NP] fp32, eps [S,B,Z] -> samples [S,B,Z], kl_rows [B,Z] or None."""
    S, B, Z = eps.shape
    samples = torch.empty((S, B, Z), dtype=torch.float32, device=params.device)
    kl = torch.empty((B, Z), dtype=torch.float32, device=params.device) if want_kl else None
    L.call("ups_latent_fwd", L.ptr(params), L.ptr(eps.contiguous()), (C.c_float * S)(*levels), S, B, Z,
           L.ptr(samples), L.ptr(kl), L.stream())
    return samples, kl


def latent_bwd(params, eps, levels, g_samples, g_kl_dev, g_kl_scale):
    S, B, Z = eps.shape
    gp = torch.empty_like(params)
    L.call("ups_latent_bwd", L.ptr(params), L.ptr(eps.contiguous()), (C.c_float * S)(*levels),
           L.ptr(g_samples.contiguous()), L.ptr(g_kl_dev), float(g_kl_scale), S, B, Z, L.ptr(gp), L.stream())
    return gp


class NoiseStream(object):
    """Standard-normal noise from the library's own Philox4x32-10 kernel (ups_randn): a (seed, offset) counter stream -- the
    values are a pure function of the seed and of how many values were drawn before, on any launch geometry."""

    def __init__(self, seed):
        self.seed, self.offset = int(seed) & ((1 << 64) - 1), 0

    def fill(self, out):
        assert out.dtype == torch.float32 and out.is_contiguous()
        n = out.numel()
        L.call("ups_randn", L.ptr(out), n, self.seed, self.offset, L.stream())
        self.offset += (n + 3) // 4
        return out

    def randn(self, *shape, device=None):
        return self.fill(torch.empty(*shape, dtype=torch.float32, device=device))


# --------------------------------------------------------------------------- guarded optimizer step (csrc/stepguard.hip)
GUARD_WORDS = 8         # a ups_step_guard record as int64 words (64 bytes)
_GUARD_SCRATCH = {}     # (device, count) -> the slab of ups_grad_guard's per-chunk partials: one per bucket size, reused every step


def guard_records(n, device):
    """n zeroed ups_step_guard records, [n, GUARD_WORDS] int64 on `device`: row i is record i (``guard_read`` decodes one)."""
    assert C.sizeof(L.StepGuard) == 8 * GUARD_WORDS
    return torch.zeros((n, GUARD_WORDS), dtype=torch.int64, device=device)


def guard_read(rec):
    """One record (a [GUARD_WORDS] int64 row, device or host) as a dict of python numbers; a device row synchronises."""
    raw = rec.detach().cpu().contiguous().numpy().tobytes()
    s = L.StepGuard.from_buffer_copy(raw)
    return {"sumsq": s.sumsq, "norm": s.norm, "scale": s.scale, "skip": s.skip, "nonfinite": s.nonfinite,
            "skipped": s.skipped_total, "clipped": s.clipped_total, "consecutive": s.consecutive}


def grad_guard(g, rec, grad_scale, clip_norm, skip_nonfinite, max_blocks=0):
    """ups_grad_guard over the flat fp32 bucket `g` on the current stream: the key's record `rec` (a row of ``guard_records``) gets this
    step's squared norm, norm of grad_scale * g, clip scale, non-finite count and skip decision, and its counters advance.  Nothing
    comes back to the host.  The scratch slab is cached per (device, count): launches of one bucket size are ordered on one stream by
    the trainer (each key's guard runs directly before its Adam)."""
    if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
        raise L.UpsError("grad_guard: a contiguous float32 device bucket is expected (got {} {})".format(tuple(g.shape), g.dtype))
    if rec.dtype != torch.int64 or rec.numel() != GUARD_WORDS or rec.device != g.device or not rec.is_contiguous():
        raise L.UpsError("grad_guard: rec is one row of guard_records on the bucket's device")
    n = g.numel()
    key = (g.device, n)
    scratch = _GUARD_SCRATCH.get(key)
    if scratch is None:
        nbytes = L.load().ups_grad_guard_scratch_bytes(n)
        if nbytes == 0:
            raise L.UpsError("grad_guard: {} elements are more than one call takes".format(n))
        scratch = _GUARD_SCRATCH[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device)
    L.call("ups_grad_guard", L.ptr(g), n, float(grad_scale), float(clip_norm), int(bool(skip_nonfinite)), L.ptr(scratch), L.ptr(rec),
           int(max_blocks), L.stream())
    return rec


def state_update_guarded(stats, old, out, decay, gain, up_loa, loa_lr, loa_target, up_lor, lor_lr, lor_target, lor_min, lor_max, skipped):
    """ups_state_update_guarded: `skipped` int64 [2] on the device = (total, consecutive)."""
    assert skipped.dtype == torch.int64 and skipped.numel() == 2
    L.call("ups_state_update_guarded", L.ptr(stats), L.ptr(old), L.ptr(out), float(decay), float(gain), int(up_loa), float(loa_lr),
           float(loa_target), int(up_lor), float(lor_lr), float(lor_target), float(lor_min), float(lor_max), L.ptr(skipped), L.stream())
    return out


def adam_step(p, g, m, v, lr_t, beta1, beta2, eps, grad_scale=1.0, guard=None):
    """lr_t: python float, or a 1-element fp32 device tensor (HIP-graph mode: the value is read on the device).  guard: the key's
    ups_step_guard record (``grad_guard`` has just filled it on this stream): ups_adam_guarded multiplies the gradient by its clip
    scale, or leaves p, m, v alone when its skip flag is set."""
    if guard is not None:
        dev_lr = torch.is_tensor(lr_t)
        L.call("ups_adam_guarded", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), 0.0 if dev_lr else float(lr_t),
               L.ptr(lr_t) if dev_lr else None, float(beta1), float(beta2), float(eps), float(grad_scale), L.ptr(guard), L.stream())
    elif torch.is_tensor(lr_t):
        L.call("ups_adam_dev", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(lr_t), float(beta1), float(beta2),
               float(eps), float(grad_scale), L.stream())
    else:
        L.call("ups_adam", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), float(lr_t), float(beta1), float(beta2),
               float(eps), float(grad_scale), L.stream())


# --------------------------------------------------------------------------- weight EMA (csrc/ema.hip)
class EmaItems(object):
    """The host array of ups_ema_item for a fixed list of (shadow, weights, rec) triples, built and validated once: `shadow` and
    `weights` flat contiguous float32 device tensors of equal length on one device (views at any 4-byte offset), `rec` the key's row
    of ``guard_records`` or None (never skipped).  Holds the tensors, so the pointers it carries stay valid."""

    def __init__(self, triples):
        triples = [tuple(t) for t in triples]
        if len(triples) > L.EMA_MAX_ITEMS:
            raise L.UpsError("ema: {} items are more than the {} one call takes".format(len(triples), L.EMA_MAX_ITEMS))
        self.tensors, self.device = triples, None
        self.array = (L.EmaItem * max(1, len(triples)))()
        for i, (s, w, rec) in enumerate(triples):
            for name, t in (("shadow", s), ("weights", w)):
                if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
                    raise L.UpsError("ema: item {}: {} must be a flat contiguous float32 device bucket (got {} {})".format(
                        i, name, tuple(t.shape), t.dtype))
            if s.numel() != w.numel() or s.device != w.device or (self.device is not None and s.device != self.device):
                raise L.UpsError("ema: item {}: shadow and weights must have one length and every item one device".format(i))
            if rec is not None and (rec.dtype != torch.int64 or rec.numel() != GUARD_WORDS or rec.device != s.device
                                    or not rec.is_contiguous()):
                raise L.UpsError("ema: item {}: rec is one row of guard_records on the buckets' device".format(i))
            self.device = s.device
            it = self.array[i]
            it.shadow, it.weights, it.count = s.data_ptr(), w.data_ptr(), s.numel()
            it.rec = rec.data_ptr() if rec is not None else None

    def __len__(self):
        return len(self.tensors)


def _ema_items(items):
    return items if isinstance(items, EmaItems) else EmaItems(items)


def ema_update(items, n_updates, omd, decay, warmup, max_blocks=0):
    """ups_ema_update on the current stream: every item's shadow moves towards its weights by this update's 1 - decay (two launches
    for all items; an item whose guard record says "skipped" keeps its shadow and its count).  items: an ``EmaItems`` or its list of
    triples; n_updates: int64 [len(items)] on the device, zeroed once by the caller; omd: float32 [len(items)] device scratch."""
    items = _ema_items(items)
    n = len(items)
    if n_updates.dtype != torch.int64 or omd.dtype != torch.float32 or n_updates.numel() != n or omd.numel() != n:
        raise L.UpsError("ema_update: n_updates is int64 [{}] and omd float32 [{}]".format(n, n))
    for t in (n_updates, omd):
        if not t.is_cuda or not t.is_contiguous() or (items.device is not None and t.device != items.device):
            raise L.UpsError("ema_update: n_updates and omd are contiguous tensors on the buckets' device")
    L.call("ups_ema_update", items.array, n, float(decay), int(bool(warmup)), L.ptr(n_updates), L.ptr(omd), int(max_blocks), L.stream())


def ema_swap(items, max_blocks=0):
    """ups_ema_swap on the current stream: shadow and weights of every item exchange their bits in place (one launch)."""
    items = _ema_items(items)
    L.call("ups_ema_swap", items.array, len(items), int(max_blocks), L.stream())


def gauss_hm(pts, stddev, h, w):
    B, K, _ = pts.shape
    out = torch.empty((B, h, w, K), dtype=torch.float32, device=pts.device)
    L.call("ups_gauss_hm", L.ptr(pts.contiguous()), L.ptr(stddev.contiguous()), L.ptr(out), B, h, w, K, L.stream())
    return out


def gauss_hm3(mu, Lt, h, w):
    B, K, _ = mu.shape
    out = torch.empty((B, h, w, K), dtype=torch.float32, device=mu.device)
    L.call("ups_gauss_hm3", L.ptr(mu.contiguous()), L.ptr(Lt.contiguous()), L.ptr(out), B, h, w, K, L.stream())
    return out
