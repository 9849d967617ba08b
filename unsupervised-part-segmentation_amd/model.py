"""``TrainModel`` / ``Trainer``: the edflow-facing surface of the reference
(cub/code/SB_model48i/model.py: TrainModel 251-521, Trainer 570-1068) on the MI355X-native path.

The reference builds a static TF graph and lets ``session.run`` execute it; here ``Trainer.train_step``
plays the role of one ``session.run(train_op)``: forward, the seven per-sub-network losses, the
per-key gradients (each sub-network is updated with the gradient of ITS OWN loss only, model.py:739-742,
786-815), TF-style Adam and the Lagrangian / EMA state updates -- all on device, no host sync.

Tape layout (cuts where the per-key semantics need different upstream gradients):
  A  encoder_0 -> latent parameters            (gets d rec, d adversarial, d bottleneck)
  B  decoder_visualize: z -> logits            (weights: d(rec + priors); input z: d rec only)
  C  hard masks -> parts -> encoder_1 -> unpool -> decoder_delta -> perceptual loss
  D  the three critics
The part path between B and C (soft-max, hard max, moments, rectangles, priors) is not taped at all:
its forward and its fused backward are single HIP kernels.
"""
import contextlib
import ctypes as C
import math
import os
import warnings
from collections import OrderedDict
from collections.abc import Mapping

import torch

from . import lib as L
from . import switches as SW
from . import nets as N
from . import ops
from . import dist as D
from . import tps as TPS
from . import stepsync as SS
from . import imglog as IL
from .nets import Act
from .schedules import make_var, make_linear_var


PERCEPTUAL_INPUTS = ("native", "resize256", "resize256_crop224")
# A/B switch (off: measured neutral, 2 032 / 2 034 against 2 017 / 2 057 img/s): enqueue the mask decoder's forward before the critics
STATE_KERNEL = SW.flag("UPS_STATE_KERNEL")          # A/B switch: the state update as one launch (ups_state_update)
STATE_KEYS = ("avg_acc0", "avg_acc1", "avg_acc_error", "avg_loss_dis0", "avg_loss_dis1", "avg_mim", "avg_independent_mim", "loa", "lor")
CRITIC_STREAMS = SW.flag("UPS_CRITIC_STREAMS")      # A/B switch: the three critics on three side streams
EARLY_ALPHA = SW.flag("UPS_EARLY_ALPHA")      # A/B switch: appearance code on "aux" beside the pose encoder


def _scalar(v, device):
    return torch.tensor(float(v), dtype=torch.float32, device=device)


class TrainModel(object):
    """Mirror of model.py:251-280: ``inputs``, ``outputs``, ``variables``, ``n_parts``."""

    def __init__(self, config, device=None, seed=None):
        self.config = config
        ema_config(config)          # (an unknown or ill-formed `ema_*` key is refused before anything is built)
        if not torch.cuda.is_available():
            raise L.UpsError("TrainModel needs a HIP device: the product path has no CPU fallback")
        L.load()
        self.device = torch.device(device if device is not None else "cuda:{}".format(torch.cuda.current_device()))
        self.pretty = config.get("use_pretty", False)
        self.n_parts = config.get("n_parts")
        self.use_tps = config.get("use_tps", False)             # model.py:334-337: in-graph TPS augmentation (tps.py, UNVERIFIED)
        self.tps_parameters = dict(config.get("tps_parameters") or {}) if self.use_tps else None
        prec = str(config.get("precision", "bf16")).lower()
        self.act_dtype = torch.float32 if prec in ("fp32", "f32", "float32") else torch.bfloat16
        # precision: fp8 (BASELINE config #5) = bf16 tensors, forward and input gradient of the wide 3x3 / stride-1 convolutions
        # with e4m3 / e5m2 MFMA operands and fp32 accumulation (ops.Fp8); weight gradients stay on the bf16 kernels
        # the fp8 state (scale slots, hand-off, switches, counters) is an object of THIS model; `fp8_copy_only: False` lets every
        # eligible layer convert its operand in the kernel (one-step runs: no producer has a delayed scale yet)
        self.fp8 = ops.Fp8.activate(ops.Fp8State(prec in ("fp8", "f8", "e4m3"), config.get("fp8_copy_only")))
        self.patch_size = config.get("patch_size", 32)
        self.df = N.is_48c(config)          # DeepFashion SB_model48c variant (two inputs, no rectangles, extra decoders)
        self.nets = N.Nets(config, self.device, seed if seed is not None else config.get("seed", 0))
        self.bank = self.nets.bank
        self._last, self._tps, self.generated_act = {}, {}, None
        self._seg_stream = None             # export_segments: the side stream of its device-to-host copies (made on first use)

    # model.py:260-263
    @property
    def inputs(self):
        B, S = self.config["batch_size"], self.config["spatial_size"]
        names = ("view0", "view1") if self.df else ("view0", "view1", "view0_target")     # SB_model48c:253
        return {k: (B, S, S, 3) for k in names}

    @property
    def variables(self):
        return self.bank.params

    # model.py:265-280 -- evaluated for the most recent batch given to ``forward``
    @property
    def outputs(self):
        out = dict(self._last)
        if self.use_tps:
            out.update(self._tps)        # model.py:272-279
        return out

    def to_act(self, x_f32, fmt=None, out=None):
        """fp32 [n,H,W,c] -> activation dtype, 8-padded channels (fmt = L.F16: fp16 in a bf16 container, ops.py).
        out: a contiguous destination of that shape (e.g. one half of a batch that two calls fill: no torch.cat)."""
        x_f32 = x_f32.contiguous()
        if out is None:
            out = torch.empty(x_f32.shape[:-1] + (ops.round8(x_f32.shape[-1]),), dtype=self.act_dtype, device=x_f32.device)
        assert out.is_contiguous() and out.shape[:-1] == x_f32.shape[:-1] and out.shape[-1] == ops.round8(x_f32.shape[-1])
        rows = x_f32.numel() // x_f32.shape[-1]
        L.call("ups_pad_convert", L.ptr(x_f32), x_f32.shape[-1], L.ptr(out), L.dt(out) if fmt is None else fmt, out.shape[-1], rows,
               L.stream())
        return out

    def latent_act(self, z_f32):
        """A latent sample [n,Z] as the mask decoder's input handle (in the decoder's tensor format)."""
        n, Z = z_f32.shape
        fmt = self.nets.scope_fmt.get("decoder_visualize")
        return Act(self.to_act(z_f32.view(n, 1, 1, Z), fmt), n, 1, 1, Z, fmt=fmt)

    def part_images(self, view_act, view_f32, hard, hard_bits):
        """The P*B part images view1[b] * hard1[b,:,:,p] in part-major order (mask_parts + apply_partwise, model.py:176-187,
        nn.py:97-103) as an activation handle for encoder_1.  Where the fused form applies (`fuse_mask_parts`, default on; bf16,
        16-aligned images, P <= 32) the [P*B,S,S,8] tensor is never built: the first convolution masks the view while it loads
        and its input gradient is reduced to d/d hard in the epilogue."""
        B, S, _, P = hard.shape
        if (hard_bits is not None and self.config.get("fuse_mask_parts", True)
                and ops.masked_conv_eligible(self.act_dtype, S, P)):
            return Act(view_act.contiguous(), P * B, S, S, 3, mask=(hard, hard_bits, view_f32))
        return Act(ops.MaskPartsFn.apply(view_f32, hard, self.act_dtype), P * B, S, S, 3)

    @torch.no_grad()
    def forward(self, batch, noise=None):
        """Inference graph (test_mode semantics when ``noise`` is None): fills ``outputs``."""
        cfg = self.config
        ops.Fp8.activate(self.fp8)
        v0 = batch["view0"].to(self.device, torch.float32)
        v1 = batch["view1"].to(self.device, torch.float32)
        B, S = v0.shape[0], v0.shape[1]
        Z, A, P = cfg.get("z0_size", 256), cfg.get("local_app_size", 64), self.n_parts
        img01 = self.to_act(torch.cat([v0, v1], 0))
        pe = self.nets.e_pi(Act(img01, 2 * B, S, S, 3)).t.view(2 * B, -1)
        if noise is None:
            z = pe[:, :Z].contiguous()
        else:
            s0, _ = ops.latent_fwd(pe[:B].contiguous(), noise["eps_pi0"][:1].to(self.device), [1.0], False)
            s1, _ = ops.latent_fwd(pe[B:].contiguous(), noise["eps_pi1"][None].to(self.device), [1.0], False)
            z = torch.cat([s0[0], s1[0]], 0)
        lm = self.nets.dv(self.latent_act(z)).t
        eps = None if noise is None else torch.cat([noise["eps_l0"], noise["eps_l1"]], 0).to(self.device)
        _, m, hard, _, bits = ops.part_softmax(lm, eps, want_bits=P <= 32)
        _, soft, _, amax = ops.part_softmax(lm[:B].contiguous(), None, want_hard=False, want_argmax=True)
        yp = self.nets.e_alpha(self.part_images(img01[B:], v1.contiguous(), hard[B:].contiguous(),
                                                None if bits is None else bits[B:].contiguous())).t
        feat = yp.float().view(P, B, A).permute(1, 0, 2).contiguous()
        inj = ops.UnpoolFn.apply(hard[:B].contiguous(), feat, self.act_dtype)
        gen = self.nets.dd(Act(inj, B, S, S, A + P)).t
        self.generated_act = gen         # the decoder's own tensor [B,S,S,8] (activation layout): what Trainer.validate hands the trunk
        self._last = {"generated": gen[..., :3].float(), "m0_sample": m[:B], "out_parts_hard": amax,
                      "out_parts_soft": soft, "view0_mask00_rgb": mask2rgb(m[:B])}
        return self._last

    # ------------------------------------------------------------------ appearance transfer (final_eval/eval_transfer.py; the
    # training graph's _cross_generated, SB_model48i/model.py:488-500).  Only unpool_features and the hourglass decoder depend on
    # the (pose, appearance) pair: n poses and m appearances are encoded once each, K = n * m combinations are decoded.  Test-mode
    # semantics as forward(batch, noise=None): latent means, no sampling noise, this model's Fp8State active.
    def _encode(self, *groups, masks=True, soft=False):
        """groups: (views [n_g,S,S,3], want_feat) -> one dict per group.  The pose path (e_pi, dv, soft-max) runs ONCE over all groups
        concatenated, as ``forward`` runs it over view0 and view1 together: the convolutions' split-K factors depend on the batch, so
        only the same batch composition gives ``forward``'s bits.  e_alpha runs per group that wants features (forward: view1).
        masks=False (``segment``): only "out_parts_hard" per group -- no hard masks, no bit sets, nothing for e_alpha to read;
        with soft=True (``segment_soft``) also "out_parts_soft", the fp32 soft-max the arg-max is taken of."""
        cfg = self.config
        ops.Fp8.activate(self.fp8)
        vs = [g[0].to(self.device, torch.float32).contiguous() for g in groups]
        v = vs[0] if len(vs) == 1 else torch.cat(vs, 0)
        n, S = v.shape[0], v.shape[1]
        Z, A, P = cfg.get("z0_size", 256), cfg.get("local_app_size", 64), self.n_parts
        img = self.to_act(v)
        pe = self.nets.e_pi(Act(img, n, S, S, 3)).t.view(n, -1)
        lm = self.nets.dv(self.latent_act(pe[:, :Z].contiguous())).t
        if masks:
            _, m, hard, _, bits = ops.part_softmax(lm, None, want_bits=P <= 32)
        _, smax, _, amax = ops.part_softmax(lm.contiguous(), None, want_hard=False, want_argmax=True)
        outs, o = [], 0
        for vg, (_, want_feat) in zip(vs, groups):
            sl = slice(o, o + vg.shape[0])
            o += vg.shape[0]
            if not masks:
                outs.append({"out_parts_hard": amax[sl], "out_parts_soft": smax[sl]} if soft else {"out_parts_hard": amax[sl]})
                continue
            out = {"hard": hard[sl].contiguous(), "out_parts_hard": amax[sl], "out_parts_soft": smax[sl], "m0_sample": m[sl]}
            if want_feat:
                yp = self.nets.e_alpha(self.part_images(img[sl], vg, out["hard"], None if bits is None else bits[sl].contiguous())).t
                out["feat"] = yp.float().view(P, vg.shape[0], A).permute(1, 0, 2).contiguous()
            outs.append(out)
        return outs

    @torch.no_grad()
    def encode_pose(self, views):
        """views [n,S,S,3] -> {"hard" [n,S,S,P] (the test-mode hard masks decode_mixed takes), "out_parts_hard", "out_parts_soft",
        "m0_sample"}: what ``forward`` computes for view0, bit for bit.  ``forward`` runs the pose path of n pairs on 2n images and the
        convolutions plan by the batch (``_encode``), so the views stand in for the view1 half as well: the pose path is paid twice
        here (transfer_matrix, which encodes rows and columns together, pays it once)."""
        return self._encode((views, False), (views, False))[0]

    @torch.no_grad()
    def segment(self, views):
        """views [n,S,S,3] -> ``out_parts_hard`` int64 [n,S,S] on the device, from the pose path alone: e_pi -> dv -> soft-max
        arg-max.  No e_alpha, no unpool, no dd -- most of a ``forward``'s FLOPs -- and no soft or hard map is kept.
        The views run in passes of at most 2 * batch_size images, each pass ONE ``_encode`` of two groups of batch_size: the batch
        ``forward`` gives the pose path.  As ``_encode`` says, the convolutions' split-K factors depend on the batch, so only the same
        batch composition gives ``forward``'s bits: for n = 2 * batch_size the first batch_size maps are the bits of
        ``forward({"view0": views[:B], "view1": views[B:]})["out_parts_hard"]``.  A shorter last pass is padded to 2 * batch_size with
        copies of its first image and the padding is dropped, so every pass plans alike.  Test-mode semantics (latent means, no
        noise).  Under precision: fp8 a pass records activation maxima like any forward."""
        return self._segment(views, False)[0]

    def _segment(self, views, want_soft):
        B = int(self.config["batch_size"])
        views = torch.as_tensor(views)
        n, S = views.shape[0], views.shape[1]
        out = torch.empty((n, S, S), dtype=torch.int64, device=self.device)
        soft = torch.empty((n, S, S, self.n_parts), dtype=torch.float32, device=self.device) if want_soft else None
        for c0 in range(0, n, 2 * B):
            v = views[c0:c0 + 2 * B].to(self.device, torch.float32)
            k = v.shape[0]
            if k < 2 * B:
                v = torch.cat([v, v[:1].expand(2 * B - k, S, S, v.shape[3])], 0)
            a, b = self._encode((v[:B], False), (v[B:], False), masks=False, soft=want_soft)
            out[c0:c0 + min(k, B)] = a["out_parts_hard"][:k]
            if k > B:
                out[c0 + B:c0 + k] = b["out_parts_hard"][:k - B]
            if want_soft:
                soft[c0:c0 + min(k, B)] = a["out_parts_soft"][:k]
                if k > B:
                    soft[c0 + B:c0 + k] = b["out_parts_soft"][:k - B]
        return out, soft

    @torch.no_grad()
    def segment_soft(self, views):
        """``segment`` that keeps the soft map: (``out_parts_hard`` int64 [n,S,S], ``out_parts_soft`` float32 [n,S,S,P]) on the device.
        The same passes of 2 * batch_size images and the same padding as ``segment``, so both are ``forward``'s bits for the batch
        composition its docstring names; the arg-max is the first maximal index of the soft map."""
        return self._segment(views, True)

    @torch.no_grad()
    def export_segments(self, views, sizes, sources=None, outputs=("labels", "overlay"), alpha=0.5, colors=None, maps=None,
                        after_launch=None, refine=None, clean=None, rle=False):
        """Part maps of `views` [n,S,S,3] rendered at their own sizes: one ``segment_soft`` and ONE ups_segment_render launch
        (``ops.segment_render``: label = first maximal part of the bilinearly resampled soft map, decided in fp64).
        sizes [(h_i, w_i)]; sources: None or n uint8 [h_i,w_i,3] images the overlay blends with (weight 1 - alpha);
        outputs: any of labels / overlay / confidence; colors uint8 [P,3] (default: the palette of the training image logs).
        maps: the (hard, soft) of an earlier ``segment_soft(views)`` (the pass is then not run again); after_launch: called once the
        kernel is launched and before the copies are queued (a profiler's lap).
        refine: None, or {"radius": R, "sigma": sigma}: the edge-aware route of ``ops.segment_render`` (joint bilateral upsampling
        guided by `sources`, which are then required and uploaded also when no overlay is wanted).
        clean: None, or {"min_area": A, "rounds": R, "connectivity": 4 | 8}: speck clean-up of the rendered labels before anything is
        copied -- up to R rounds of ``ops.label_components`` -> ``label_component_stats`` -> ``label_components_clean`` on the packed
        labels plane, in place: a component of fewer than A pixels takes the label its edge neighbours vote for; overlay, confidence
        (0 at a relabelled pixel) and the counts follow.  One int32 is read per round (it ends the rounds when nothing changed);
        "relabelled" in the result is the number of pixels that changed.
        rle: True also run-length encodes the FINAL labels (after refinement and clean-up) with ``ops.segment_rle`` -- one more int64
        read -- and `host` gains "rle_offsets" int64 [n P + 1], "rle_counts" int32, "area" int32 [n,P] and "bbox" int32 [n,P,4], copied
        on the same side stream behind the same event (``ops.rle_lists`` splits them); `outputs` may then be empty.
        The per-part pixel counts are always taken.  The planes are copied into pinned host buffers on a side stream behind an event
        (as the image logs' canvases): nothing here waits for the device.  Returns {"table", "total", "host": {name: pinned
        tensor, "counts" included}, "views": {name: [per-image host views]}, "ready": the copies' event, "soft", "hard": the device
        maps of ``segment_soft``}: read the host buffers after ``ready.synchronize()``."""
        outputs = tuple(outputs)
        if (not outputs and not rle) or any(k not in ("labels", "overlay", "confidence") for k in outputs):
            raise L.UpsError("export_segments: outputs is a non-empty subset of labels / overlay / confidence (got {})".format(outputs))
        dev = self.device
        hard, soft = self.segment_soft(views) if maps is None else maps
        if colors is None and "overlay" in outputs:
            colors = IL.mask_color_bytes(IL.mask_colors01(self.n_parts))
        src = sources if "overlay" in outputs or refine is not None else None
        want = outputs + ("counts",)
        if clean is not None:
            if src is not None and not torch.is_tensor(src):    # the clean-up blends from the packed sources too: packed once, here
                table, total = ops.segment_table(sizes)
                src = ops.segment_pack_sources(src, table, total).to(dev, non_blocking=True)
        if (clean is not None or rle) and "labels" not in want:
            want = want + ("labels",)
        res = ops.segment_render(soft, sizes, src=src, colors=colors, alpha=alpha, want=want, refine=refine)
        relabelled = self._clean_segments(res, src, colors, alpha, clean) if clean is not None else 0
        if rle:
            enc = ops.segment_rle(res["labels"], self.n_parts, table=(res["table"], res["table_dev"], res["total"]))
            res.update(rle_offsets=enc["offsets"], rle_counts=enc["counts"], area=enc["area"], bbox=enc["bbox"])
        if after_launch is not None:
            after_launch()
        if self._seg_stream is None:
            self._seg_stream = torch.cuda.Stream(dev)
        main, side = torch.cuda.current_stream(dev), self._seg_stream
        side.wait_stream(main)
        host = OrderedDict()
        with torch.cuda.stream(side):
            for k in outputs + ("counts",) + (("rle_offsets", "rle_counts", "area", "bbox") if rle else ()):
                res[k].record_stream(side)
                host[k] = torch.empty(res[k].shape, dtype=res[k].dtype, pin_memory=True)
                host[k].copy_(res[k], non_blocking=True)
            ready = side.record_event()
        return {"table": res["table"], "total": res["total"], "host": host, "ready": ready, "soft": soft, "hard": hard,
                "views": {k: ops.segment_views(host[k], res["table"]) for k in outputs}, "relabelled": relabelled}

    def _clean_segments(self, res, src, colors, alpha, clean):
        """``export_segments``' clean-up rounds on the planes of a ``segment_render`` result, in place -> the pixels relabelled."""
        if not isinstance(clean, dict) or set(clean) != {"min_area", "rounds", "connectivity"}:
            raise L.UpsError("export_segments: clean is None or {{'min_area', 'rounds', 'connectivity'}} (got {!r})".format(clean))
        rounds = clean["rounds"]
        if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 4:
            raise L.UpsError("export_segments: clean rounds is an integer in 1 .. 4 (got {!r})".format(rounds))
        table, P = (res["table"], res["table_dev"], res["total"]), self.n_parts
        err, total = None, 0
        for _ in range(rounds):
            comp, err = ops.label_components(res["labels"], P, conn=clean["connectivity"], table=table, err=err)
            area, _, _ = ops.label_component_stats(res["labels"], comp, P, table=table)
            _, changed = ops.label_components_clean(res["labels"], comp, area, P, clean["min_area"], table=table, out=res["labels"],
                                                    src=src, colors=colors, alpha=alpha, overlay=res.get("overlay"),
                                                    confidence=res.get("confidence"), counts=res["counts"])
            moved = int(changed.item())                 # the one int32 read of the round
            total += moved
            if moved == 0:
                break
        ops.components_check(err)
        return total

    @torch.no_grad()
    def encode_appearance(self, views):
        """views [m,S,S,3] -> part appearances [m,P,A] fp32: each view masked by ITS OWN test-mode hard masks, through part_images /
        e_alpha as ``forward`` does for view1 (the second half of a pose batch of 2m, as there: see encode_pose)."""
        return self._encode((views, False), (views, True))[1]["feat"]

    @torch.no_grad()
    def encode_parts(self, views):
        """views [n,S,S,3] -> {"feat" [n,P,A] fp32 (one appearance code per image and part, as ``encode_appearance``), "area" [n,P]
        int32 (the pixels of ``out_parts_hard`` equal to p: ``ops.part_usage``'s counts), "out_parts_hard" int64 [n,S,S]} on the
        device: the bank of ``partindex.PartIndex``.  Passes of 2 * batch_size images, ONE ``_encode((v[:B], True), (v[B:], True))``
        each -- the batch ``forward`` gives the pose path, so the convolutions plan alike, and the pose path is paid once, not twice
        as in ``encode_appearance``.  A shorter last pass is padded with copies of its first image, as in ``segment``, and the
        padding is dropped.  Test-mode semantics.  Under precision: fp8 a pass records activation maxima like any forward."""
        B, P = int(self.config["batch_size"]), self.n_parts
        views = torch.as_tensor(views)
        n, S = views.shape[0], views.shape[1]
        feat = torch.empty((n, P, int(self.config.get("local_app_size", 64))), dtype=torch.float32, device=self.device)
        area = torch.zeros((n, P), dtype=torch.int32, device=self.device)
        hard = torch.empty((n, S, S), dtype=torch.int64, device=self.device)
        for c0 in range(0, n, 2 * B):
            v = views[c0:c0 + 2 * B].to(self.device, torch.float32)
            k = v.shape[0]
            if k < 2 * B:
                v = torch.cat([v, v[:1].expand(2 * B - k, S, S, v.shape[3])], 0)
            for o, g in zip((0, B), self._encode((v[:B], True), (v[B:], True))):
                m = min(k - o, B)
                if m > 0:
                    feat[c0 + o:c0 + o + m] = g["feat"][:m]
                    hard[c0 + o:c0 + o + m] = g["out_parts_hard"][:m]
                    ops.part_usage(g["out_parts_soft"][:m].contiguous(), g["out_parts_hard"][:m].contiguous(),
                                   counts=area[c0 + o:c0 + o + m])
        return {"feat": feat, "area": area, "out_parts_hard": hard}

    @torch.no_grad()
    def part_centres(self, views, source="soft", min_part_area=0.005):
        """views [n,S,S,3] -> {"centre" [n,P,2] float64 ((x, y) of each part's centre on [-1, 1], pixel centres at (2x + 1) / S - 1),
        "mass" [n,P] float64, "valid" [n,P] uint8, "out_parts_hard" int64 [n,S,S]} on the device: the features of
        ``landmarks.LandmarkRegressor``.  The same passes of 2 * batch_size images and the same padding as ``segment_soft``, one
        ups_part_moments launch pair per pass (``ops.part_moments``; definitions: include/upsparts_hip.h).
        source "soft": mass = the sum of out_parts_soft, centre = its mean position, valid = mass >= min_part_area * S^2.
        source "hard": mass = the pixels of out_parts_hard equal to p, centre = sum(2x + 1 - S) / (S * count) from the kernel's integer
        sums in float64 (one multiplication, one division), valid = count >= ceil(min_part_area * S^2) and count > 0.
        A part that is not valid has the centre (0, 0)."""
        if source not in ("soft", "hard"):
            raise L.UpsError("part_centres: source is soft | hard (got {!r})".format(source))
        B, P = int(self.config["batch_size"]), self.n_parts
        views = torch.as_tensor(views)
        n, S = views.shape[0], views.shape[1]
        out = {"centre": torch.empty((n, P, 2), dtype=torch.float64, device=self.device),
               "mass": torch.empty((n, P), dtype=torch.float64, device=self.device),
               "valid": torch.empty((n, P), dtype=torch.uint8, device=self.device),
               "out_parts_hard": torch.empty((n, S, S), dtype=torch.int64, device=self.device)}
        for c0 in range(0, n, 2 * B):
            hard, soft = self._segment(views[c0:c0 + 2 * B], True)
            k = hard.shape[0]
            out["out_parts_hard"][c0:c0 + k] = hard
            r = ops.part_moments(soft, hard if source == "hard" else None, min_mass=float(min_part_area) * S * S)
            if source == "hard":
                cnt = r["hard"][..., 0].to(torch.float64)
                ok = (cnt > 0) & (cnt >= float(math.ceil(float(min_part_area) * S * S)))
                den = torch.where(ok, cnt, torch.ones_like(cnt)) * float(S)
                centre = r["hard"][..., 1:].to(torch.float64) / den[..., None]
                centre = torch.where(ok[..., None], centre, torch.zeros_like(centre))
                r = {"centre": centre, "mass": cnt, "valid": ok.to(torch.uint8)}
            for key in ("centre", "mass", "valid"):
                out[key][c0:c0 + k] = r[key]
        return out

    @torch.no_grad()
    def decode_mixed(self, hard, feat, pose_idx, app_idx, chunk=None):
        """generated [K,S,S,3] fp32: image k has the masks hard[pose_idx[k]] and, for part p, the appearance feat[app_idx[k][p]][p].
        pose_idx [K], app_idx [K,P]: host integers.  Decoded in chunks of at most `chunk` images (default: the config's batch_size;
        the last chunk may be shorter), so the memory in flight is that of one ordinary forward."""
        ops.Fp8.activate(self.fp8)
        pi = torch.as_tensor(pose_idx, device="cpu").reshape(-1)
        P, A = self.n_parts, feat.shape[-1]
        ai = torch.as_tensor(app_idx, device="cpu").reshape(-1, P)
        K, S = pi.numel(), hard.shape[1]
        chunk = int(chunk or self.config["batch_size"])
        if K == 0 or ai.shape[0] != K or chunk < 1:
            raise L.UpsError("decode_mixed: pose_idx [K >= 1], app_idx [K,{}], chunk >= 1 (got K = {}, {} index rows, chunk {})".format(
                P, K, ai.shape[0], chunk))
        out = torch.empty((K, S, S, 3), dtype=torch.float32, device=self.device)
        for c0 in range(0, K, chunk):
            c1 = min(K, c0 + chunk)
            inj = ops.unpool_mix(hard, feat, pi[c0:c1], ai[c0:c1], self.act_dtype)
            out[c0:c1] = self.nets.dd(Act(inj, c1 - c0, S, S, A + P)).t[..., :3].float()
        return out

    @torch.no_grad()
    def transfer_matrix(self, row_views, col_views, parts=None):
        """The comparison matrix of eval_transfer.py from one pass: generated [n,m,S,S,3], cell (i, j) = pose of row image i with the
        part appearances of column image j.  parts=None: every part from j.  parts=[..]: only those parts from j, the others from
        the row image's own appearance (the rows are then appearance-encoded too).  Index layout: ``transfer_indices``."""
        n, m = row_views.shape[0], col_views.shape[0]
        rows, cols = self._encode((row_views, parts is not None), (col_views, True))
        feat = cols["feat"] if parts is None else torch.cat([rows["feat"], cols["feat"]], 0)
        pi, ai = transfer_indices(n, m, self.n_parts, parts)
        gen = self.decode_mixed(rows["hard"], feat, pi, ai)
        return {"generated": gen.view(n, m, *gen.shape[1:]),
                "row_parts_hard": rows["out_parts_hard"], "col_parts_hard": cols["out_parts_hard"],
                "row_mask_rgb": mask2rgb(rows["m0_sample"]), "col_mask_rgb": mask2rgb(cols["m0_sample"])}

    @torch.no_grad()
    def cross_generated(self, batch):
        """_cross_generated (SB_model48i/model.py:488-500) in test mode: pose of view0[k] with the appearance of view1[B-1-k]."""
        rows, cols = self._encode((batch["view0"], False), (batch["view1"], True))
        feat = cols["feat"]
        pi, ai = reversed_indices(feat.shape[0], self.n_parts)
        return self.decode_mixed(rows["hard"], feat, pi, ai)


def transfer_indices(n_rows, n_cols, n_parts, parts=None):
    """(pose_idx [K], app_idx [K,P]) int64 host tensors of an n_rows x n_cols transfer matrix, K = n_rows * n_cols, cell
    k = i * n_cols + j (row-major).  pose_idx[k] = i.  The appearance table the indices point into is
      parts=None : the column images alone             -> app_idx[k, :] = j
      parts=[..] : the row images, then the column ones -> app_idx[k, p] = n_rows + j for p in parts, i (the row's own) otherwise."""
    n, m, P = int(n_rows), int(n_cols), int(n_parts)
    i = torch.arange(n, dtype=torch.int64).repeat_interleave(m)
    j = torch.arange(m, dtype=torch.int64).repeat(n)
    if parts is None:
        return i, j[:, None].expand(n * m, P).contiguous()
    parts = sorted(set(int(p) for p in parts))
    if any(p < 0 or p >= P for p in parts):
        raise ValueError("parts {} out of range for {} parts".format(parts, P))
    app = i[:, None].expand(n * m, P).clone()
    app[:, parts] = (n + j)[:, None]
    return i, app


def reversed_indices(batch, n_parts):
    """_cross_generated: image k keeps its pose and takes every part appearance from image batch-1-k."""
    k = torch.arange(int(batch), dtype=torch.int64)
    return k, (int(batch) - 1 - k)[:, None].expand(int(batch), int(n_parts)).contiguous()


def mask_colors(n_parts):
    """nn.py:2118-2120 (inferno colour table); needs matplotlib, falls back to a grey ramp."""
    try:
        from matplotlib import pyplot as plt
        import numpy as np
        return torch.tensor(plt.cm.inferno(np.linspace(0, 1, n_parts))[:, :3], dtype=torch.float32)
    except Exception:  # pragma: no cover
        return torch.linspace(0, 1, n_parts).view(-1, 1).repeat(1, 3)


def mask2rgb(mask):
    """nn.py:2067-2089: one-hot(argmax) x colours in [-1,1] (visualisation output only)."""
    P = mask.shape[3]
    col = ((mask_colors(P) - 0.5) * 2).to(mask.device)
    return col[mask.argmax(dim=3)]


class _Step(object):
    """The tensors and constants of one training step, handed from segment to segment (Trainer._step_begin ... _log_thunk)."""


class _LazyLosses(Mapping):
    """What train_step returns: the per-key losses OF THAT STEP, computed when first read and cached (the object keeps the step's
    own thunk, so reading it after later steps still yields this step's values).  A read-only Mapping (dict(x), json via
    dict(x), isinstance(x, Mapping) work)."""

    def __init__(self, trainer):
        self._t, self._thunk = trainer, trainer._lazy_logs
        # (HIP-graph mode computes the values with the step, into buffers every replay overwrites: nothing to defer)
        self._vals = trainer._losses if self._thunk is None else None

    def _d(self):
        if self._vals is None:
            t = self._t
            if t._lazy_logs is self._thunk:
                self._vals = t.losses                   # still the trainer's latest step: materialise there (log_ops share it)
            elif t._done_thunk is self._thunk:
                self._vals = t._losses                  # ... which somebody has already done
            else:
                self._vals = self._thunk()[0]           # later steps have replaced the trainer's view: evaluate this step's own
            self._thunk = None
        return self._vals

    def __getitem__(self, k):
        return self._d()[k]

    def __iter__(self):
        return iter(self._d())

    def __len__(self):
        return len(self._d())


def gram_weight_of(config, logger=None):
    """`gram_weight` (model.py:608, edflow VGG19Features(default_gram=...)): a plain number passed to the constructor, not a make_var
    schedule; default 0.0 in every shipped yaml.  edflow adds the Gram terms only when the weight is > 0: 0 or below means none."""
    v = config.get("gram_weight", 0.0)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("gram_weight: a number is expected (got {!r}); it is not a make_var schedule".format(v))
    v = float(v)
    if v < 0:
        msg = "gram_weight {} < 0: no Gram terms (edflow adds them only for a positive weight)".format(v)
        if logger:
            logger.warning(msg)
        else:
            warnings.warn(msg)
    return v if v > 0 else 0.0


VAL_METRICS = ("iou", "reconstruction", "parts", "equivariance")
VAL_METRICS_MORE = ("coherence",)       # accepted beside VAL_METRICS, and ordered after them
VAL_METRICS_ALL = VAL_METRICS + VAL_METRICS_MORE


def validation_metrics(config, key="val_metrics", default=("iou",)):
    """The metric names of `val_metrics` (default ["iou"]: the part IoU alone, which needs label images) or of the runner's
    `eval_metrics` (default none); ValueError on an unknown name, and on an empty `val_metrics`."""
    v = config.get(key)
    if v is None:
        return list(default)
    if isinstance(v, str) or not isinstance(v, (list, tuple)):
        raise ValueError("{}: a list drawn from {} is expected (got {!r})".format(key, " | ".join(VAL_METRICS_ALL), v))
    unknown = [m for m in v if m not in VAL_METRICS_ALL]
    if unknown:
        raise ValueError("{}: unknown metric(s) {} ({})".format(key, unknown, " | ".join(VAL_METRICS_ALL)))
    if not v and key == "val_metrics":
        raise ValueError("val_metrics is empty: with val_freq set, list at least one of {}".format(" | ".join(VAL_METRICS_ALL)))
    return [m for m in VAL_METRICS_ALL if m in v]


def coherence_config(config):
    """The keys of the `coherence` metric, decided from the config alone -> (connectivity, speck area in pixels of the S x S part map):
    `val_coherence_connectivity` (8; 4 or 8) and `val_speck_area` (0.001: a share of S^2 like `val_min_part_area`, converted with ceil;
    a component of fewer pixels is a speck).  ValueError with the reason."""
    conn = config.get("val_coherence_connectivity", 8)
    if isinstance(conn, bool) or conn not in (4, 8):
        raise ValueError("val_coherence_connectivity: 4 or 8 is expected (got {!r})".format(conn))
    share = config.get("val_speck_area", 0.001)
    if isinstance(share, bool) or not isinstance(share, (int, float)) or not 0.0 <= share <= 1.0:
        raise ValueError("val_speck_area: a share of the map in [0, 1] is expected (got {!r})".format(share))
    S = int(config.get("spatial_size", 256))
    return int(conn), int(math.ceil(float(share) * S * S))


def equivariance_tps_parameters(config):
    """The warp block of the `equivariance` metric: `val_equivariance_tps`, else the yaml's `tps_parameters` (with or without
    `use_tps`), else the block the shipped CUB yaml carries (configs.TPS_PARAMETERS)."""
    from .configs import TPS_PARAMETERS
    p = config.get("val_equivariance_tps") or config.get("tps_parameters") or TPS_PARAMETERS
    missing = [k for k in ("scal", "tps_scal", "rot_scal", "off_scal", "scal_var") if k not in p]
    if missing:
        raise ValueError("val_equivariance_tps / tps_parameters: missing key(s) {}".format(missing))
    return dict(p)


def check_validation_config(config):
    """The refusals of `val_freq` (ValueError with the reason), decided from the config alone, before anything touches the device."""
    if not int(config.get("val_freq", 0) or 0):
        return
    if str(config.get("precision", "bf16")).lower() in ("fp8", "f8", "e4m3"):
        raise ValueError("val_freq cannot be combined with precision: fp8: the model's forward records activation maxima into "
                         "its delayed-scaling slots, so a validation pass would move the next training step's scales")
    if bool(config.get("hip_graph", SW.flag("UPS_GRAPH"))):
        raise ValueError("val_freq cannot be combined with hip_graph: True: eager launches between replays of the captured "
                         "step have not been shown safe")
    metrics = validation_metrics(config)
    if "iou" in metrics and (not config.get("val_csv") or not config.get("data_gt_segmentation_column")):
        raise ValueError("val_freq needs `val_csv` and `data_gt_segmentation_column` (the csv column with the label images)")
    if not config.get("val_csv"):
        raise ValueError("val_freq needs `val_csv`")
    if "reconstruction" in metrics and int(config.get("spatial_size", 256)) < 11:
        raise ValueError("val_metrics: reconstruction needs spatial_size >= 11, the 11 x 11 SSIM window (got {})".format(
            config.get("spatial_size")))
    if "equivariance" in metrics:
        equivariance_tps_parameters(config)
    if "coherence" in metrics:
        coherence_config(config)


def step_guard_config(config):
    """The keys of the guarded optimizer step, decided from the config alone -> (grad_clip_norm, skip_nonfinite,
    nonfinite_max_consecutive); ValueError with the reason for a negative or non-finite `grad_clip_norm` and for a
    `nonfinite_max_consecutive` below 1."""
    clip = config.get("grad_clip_norm", 0.0)
    if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not math.isfinite(clip) or clip < 0:
        raise ValueError("grad_clip_norm: a finite number >= 0 is expected, 0 = no clipping (got {!r})".format(clip))
    skip = config.get("skip_nonfinite", False)
    if not isinstance(skip, bool):
        raise ValueError("skip_nonfinite: True or False is expected (got {!r})".format(skip))
    maxc = config.get("nonfinite_max_consecutive", 10)
    if isinstance(maxc, bool) or not isinstance(maxc, int) or maxc < 1:
        raise ValueError("nonfinite_max_consecutive: an integer >= 1 is expected (got {!r})".format(maxc))
    return float(clip), skip, maxc


EMA_KEYS = ("ema_decay", "ema_warmup")


def ema_config(config):
    """The keys of the weight EMA, decided from the config alone -> (ema_decay, ema_warmup, val_use_ema, use_ema);
    ValueError with the reason for an `ema_decay` outside [0, 1) (0 = off), for an unknown `ema_*` key and for `val_use_ema` without
    `ema_decay`."""
    unknown = sorted(k for k in config if isinstance(k, str) and k.startswith("ema_") and k not in EMA_KEYS)
    if unknown:
        raise ValueError("unknown weight-EMA key(s) {} ({})".format(unknown, " | ".join(EMA_KEYS)))
    decay = config.get("ema_decay", 0.0)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= decay < 1.0):     # (NaN fails both comparisons)
        raise ValueError("ema_decay: a number in [0, 1) is expected, 0 = no weight EMA (got {!r})".format(decay))
    flags = []
    for k, default in (("ema_warmup", True), ("val_use_ema", False), ("use_ema", False)):
        v = config.get(k, default)
        if not isinstance(v, bool):
            raise ValueError("{}: True or False is expected (got {!r})".format(k, v))
        flags.append(v)
    if flags[1] and not decay > 0:
        raise ValueError("val_use_ema: True needs ema_decay > 0 (there are no shadow weights to validate on)")
    return (float(decay),) + tuple(flags)


def checkpoint_shadows(ck, use_ema, where):
    """The "ema" entry of a native checkpoint dict ({"params": {name: tensor}, "n": {key: int}}) or None; ValueError under `use_ema`
    when the file holds none."""
    ema = ck.get("ema")
    if ema is not None and not ema.get("params"):
        ema = None
    if use_ema and ema is None:
        raise ValueError("use_ema: True, but {} holds no shadow weights (it was written without ema_decay)".format(where))
    return ema


class Trainer(object):
    """Mirror of model.py:570-1068 plus the pieces edflow's TFBaseTrainer supplied (session loop,
    one Adam per loss key over the variables whose name contains the key, logging cadence)."""

    def __init__(self, config, root=None, model=None, **kwargs):
        self.config, self.root, self.model = config, root, model
        check_validation_config(config)
        self.device = model.device
        self.logger = kwargs.get("logger")
        self.global_step = 0
        self._log_ops, self.img_ops, self.update_ops = OrderedDict(), OrderedDict(), []
        self.world_size = kwargs.get("world_size", 1)
        self.rank = kwargs.get("rank", 0)
        self.process_group = kwargs.get("process_group")
        self.beta1 = config.get("beta1", 0.5)        # edflow TFBaseTrainer defaults (UNVERIFIED)
        self.beta2 = config.get("beta2", 0.9)
        # Global optimizer knobs beyond the yaml (all optimizers alike; defaults = tf.train.AdamOptimizer's epsilon, no warm-up, no
        # clipping).  They exist so that hypotheses about edflow's TFBaseTrainer (source absent) are config keys, not patches:
        # tools/pin_log.py sweeps them against the reference's training log.
        self.adam_eps = float(config.get("adam_eps", 1e-8))
        self.lr_warmup_steps = int(config.get("lr_warmup_steps", 0))       # linear ramp of lr over the first N global steps
        # grad_clip_norm: per optimizer key, global L2 norm (0 = off).  skip_nonfinite: a key whose gradient holds NaN / inf does not step
        # (decided on the device, per key); nonfinite_max_consecutive: that many skipped steps in a row end the run
        self.grad_clip_norm, self.skip_nonfinite, self.nonfinite_max_consecutive = step_guard_config(config)
        # `probe`: DIAGNOSTIC hooks (tools/pin_log.py, the conditional-pin test) -- never set by a shipped config:
        #   lr_scale: {optimizer key: factor}  that key alone steps with factor * lr
        #   rec_scale: s                        decoder_visualize's gradient sees priors + s * (reconstruction term), M:786-797
        self.probe = dict(config.get("probe") or {})
        unknown = set(self.probe) - {"lr_scale", "rec_scale"}
        if unknown:
            raise ValueError("probe: unknown hook(s) {}".format(sorted(unknown)))
        self.perceptual_input = config.get("perceptual_input", "native")
        self.gram_weight = gram_weight_of(config, self.logger)
        if config.get("use_pretty", False) or config.get("add_pretty", False):
            raise NotImplementedError("the 'pretty' image discriminator (model.py:190-212) is not used by the shipped configs")
        vw = config.get("vgg_widths", N.VGG_WIDTHS)
        self.vgg = N.VggTrunk(self.device, seed=config.get("vgg_seed", 7), widths=tuple(vw),
                              post_storage=model.nets.post_storage,
                              # (measured, round 5: the trunk on fp8 copies -- 20 more launches per step on e4m3 operands -- runs the
                              # step 1.4 % SLOWER: the pools' and the convolutions' copy emission costs more than blocks 2-4 gain at
                              # 64 images; off by default, `vgg_fp8: True` for measurements)
                              fp8=bool(config.get("vgg_fp8", False)))
        # `vgg_weights`: npz / torch file with the Keras VGG19 ImageNet kernels in HWIO (edflow downloads them at run time;
        # they are not obtainable offline).  Without it the perceptual loss runs on seeded He-normal stand-ins: fine for
        # timing and parity, NOT for training a model that should match the reference's part quality -- say so loudly.
        if config.get("vgg_weights"):
            self.vgg.load(N.read_vgg_weights(config["vgg_weights"]))
            self.vgg_pretrained = True
        else:
            self.vgg_pretrained = False
            msg = ("perceptual trunk runs on seeded stand-in weights (no `vgg_weights` in the config): losses are not the "
                   "reference's ImageNet-VGG19 perceptual loss")
            if self.logger:
                self.logger.warning(msg)
            elif root is not None and self.rank == 0:
                import sys
                sys.stderr.write("[WARNING] " + msg + "\n")
        mi = config["MI"]
        d = self.device
        # non-trainable state (model.py:503, 829-834, 861-866, 890, 921) -- device scalars
        self.state = {"lon": _scalar(1.0, d), "loa": _scalar(mi.get("loa_init", 0.0), d),
                      "lor": _scalar(mi.get("lor_init", 7.5), d),
                      "avg_acc0": _scalar(0.5, d), "avg_acc1": _scalar(0.5, d), "avg_acc_error": _scalar(0.0, d),
                      "avg_loss_dis0": _scalar(1.0, d), "avg_loss_dis1": _scalar(1.0, d),
                      "avg_mim": _scalar(0.0, d), "avg_independent_mim": _scalar(0.0, d)}
        self._gen = torch.Generator(device=d)
        self._gen.manual_seed(D.shard_seed(config.get("noise_seed", 4321), kwargs.get("rank", 0)))      # TPS uniforms, crop window
        self._noise = ops.NoiseStream(D.shard_seed(config.get("noise_seed", 4321), kwargs.get("rank", 0)))  # the sampling noise
        # `use_tps`: samples whose TPS system was singular and got the identity transform (ups_tps_solve), counted on the device and read
        # on the steps that log scalars (`_check_tps_singular`: one warning per run)
        self._tps_singular = torch.zeros(1, dtype=torch.int32, device=d) if model.use_tps else None
        self._tps_warned = False
        if model.use_tps:
            TPS.base_points(d)          # (made before any capture: a captured step only launches)
        self._lazy_logs, self._done_thunk, self._last_ckpt = None, None, None
        self.switches_report = SW.report()       # the environment switches that differ from their defaults (switches.py), logged once
        if self.logger:
            self.logger.info(self.switches_report)
        # the gradient hand-off of the running step (the keys that have stepped ...); a stepsync.StepGraph once graph mode is used
        self.sync, self.graph = SS.GradSync(self), None
        # `stream_plan` (full | compact | auto): how the step's logical streams map onto HIP streams (ops.Streams.set_plan).  auto =
        # full on one rank, compact under data parallelism, where the collectives' stream needs a hardware queue of its own
        # (measured with a stand-in for the collectives on one GPU: tools/probes/stream_dp.py, profiles/round5_stream_dp.txt)
        plan = str(config.get("stream_plan", SW.value("UPS_STREAM_PLAN"))).lower()
        if plan == "auto":
            plan = "compact" if (self.world_size > 1 or D.FORCE_COLLECTIVES) else "full"
        self.stream_plan = plan
        ops.Streams.set_plan(plan)
        self._poisoned = None           # set when a step failed half-way through its optimizer updates (_after_failed_step)
        self._losses = OrderedDict((k, None) for k in self.loss_keys())
        self._graph_enabled = bool(config.get("hip_graph", SW.flag("UPS_GRAPH")))
        # the guarded optimizer step: one ups_step_guard record per optimizer key and the state update's two counters, allocated ONCE at
        # fixed addresses (never from a graph's pool: a captured step writes where guard_report reads).  Per process, from 0: checkpoints
        # do not carry them.
        self._guard_index = dict((k, i) for i, k in enumerate(self.loss_keys()))
        self._guard_rec = ops.guard_records(len(self._guard_index), d)
        self._guard_state = torch.zeros(2, dtype=torch.int64, device=d)
        self._guard_used, self._nonfinite_warned = False, False
        model.fp8.skip_nonfinite = self.skip_nonfinite        # `log_images` (default off): the reference's img_ops (model.py:968-1053) as uint8 canvases on the steps that log scalars
        self.log_images = bool(config.get("log_images", False))
        # weight EMA (default off): with `ema_decay` > 0 one shadow bucket per optimizer key, updated by ONE
        # ops.ema_update at the end of every step; allocated once at fixed addresses, as the guard records are (a captured step writes them)
        self.ema_decay, self.ema_warmup, self.val_use_ema, self.use_ema = ema_config(config)
        self._ema = None
        if self.ema_decay > 0:
            self._ema_init()
        self._want_images = False       # set for the duration of a train_step(..., images=True)
        # `val_freq: K` with `val_csv`: the metrics of `val_metrics` (default: the part IoU) on a validation csv after every K-th step
        # (``validate``)
        self.val_freq = int(config.get("val_freq", 0) or 0)
        self._val, self._val_logs = None, OrderedDict()
        if self.val_freq > 0:
            self._init_validation()
        self._img = None                # side stream, colour tables, writer: created by the first image step
        self._img_hold = None           # (sources, event) of canvases still being rendered: released when the next step begins

    # ------------------------------------------------------------------ losses / log scalars, materialised on first use
    def _set_logs(self, losses, log):
        self._losses, self._log_ops, self._lazy_logs = losses, log, None

    def _materialize(self):
        if self._lazy_logs is not None:
            thunk, self._lazy_logs = self._lazy_logs, None
            self._losses, self._log_ops = thunk()
            self._done_thunk = thunk

    @property
    def losses(self):
        self._materialize()
        return self._losses

    @property
    def log_ops(self):
        self._materialize()
        return self._log_ops

    @log_ops.setter
    def log_ops(self, value):
        self._log_ops = value

    # ------------------------------------------------------------------ edflow hook surface
    def loss_keys(self):
        keys = list(N.submodules(self.config))
        for k in self.config.get("fix_weights", []):      # model.py:1062-1067
            if k in keys:
                keys.remove(k)
        return keys

    def make_loss_ops(self):
        """model.py:604: returns {optimizer key: loss}.  In this eager design the values are the
        device scalars of the most recent step (None before the first step)."""
        return self.losses

    def get_restore_variables(self):
        """model.py:571-590: name-substring exclude list."""
        vs = list(self.model.variables.keys())
        default_exclude = ["pretty_discriminator", "beta1_power_7", "beta2_power_7", "phase_weight", "grad_weight",
                           "phase_gamma"]
        for name in self.config.get("restore_exclude", default_exclude):
            vs = [v for v in vs if name not in v]
        return vs

    def set_global_step(self, step):
        self.global_step = int(step)

    def initialize(self, checkpoint_path=None):
        """model.py:592-602: lazy restore, missing variables ignored, step parsed from the file name."""
        if checkpoint_path is None:
            return
        from . import tfckpt
        if tfckpt.is_bundle(checkpoint_path):
            return self._initialize_from_tf(checkpoint_path)
        ck = torch.load(checkpoint_path, map_location="cpu")
        ema = checkpoint_shadows(ck, self.use_ema, checkpoint_path)      # (`use_ema` with a file that holds none: refused before anything is loaded)
        keep = set(self.get_restore_variables())
        self.model.bank.load({n: t for n, t in ck["params"].items() if n in keep})
        for key, grp in self.model.bank.groups.items():
            st = ck.get("adam", {}).get(key)
            if st is not None and st["m"].numel() == grp["flat"]["m"].numel():
                grp["flat"]["m"].copy_(st["m"]); grp["flat"]["v"].copy_(st["v"]); grp["t"] = st["t"]
        for k, v in ck.get("state", {}).items():
            if k in self.state:
                self.state[k].fill_(float(v))
        self._restore_ema(ema["params"] if ema else None, ema.get("n") if ema else None, keep, checkpoint_path)
        if "noise_offset" in ck:
            self._noise.offset = int(ck["noise_offset"])
        if "gen_state" in ck:
            # The generator is seeded PER RANK (shard_seed) and only rank 0 writes checkpoints: its state is restored on the rank and
            # world size that wrote it only.  Every other rank (and any restore under a different world size) re-seeds with its own
            # shard seed advanced by the restored step, so that the ranks keep drawing DIFFERENT TPS uniforms / crop windows
            # (round-5 advisor: all ranks used to resume with rank 0's stream).
            same = int(ck.get("rank", 0)) == self.rank and int(ck.get("world_size", 1)) == self.world_size
            restored = False
            if same:
                try:
                    self._gen.set_state(ck["gen_state"])
                    restored = True
                except Exception:       # a state written on another device type / torch build
                    pass
            if not restored:
                self._gen.manual_seed(D.shard_seed(self.config.get("noise_seed", 4321), self.rank) + 1000003 * (1 + int(ck.get("global_step", 0))))
        base = os.path.basename(checkpoint_path)
        digits = "".join(ch for ch in base.split("-")[-1] if ch.isdigit())
        # the stored step is authoritative (it agrees with the restored Adam t); the file name is the fallback (model.py:597-601)
        self.set_global_step(int(ck["global_step"]) if "global_step" in ck else (int(digits) if digits else 0))
        if self.logger:
            self.logger.info("Lazily restored from {}".format(checkpoint_path))

    TF_UNNAMED_ORDER = ("lon", "avg_acc0", "avg_acc1", "avg_acc_error", "avg_loss_dis0", "avg_loss_dis1", "avg_mim",
                        "avg_independent_mim", "loa", "lor")

    def tf_unnamed_order(self):
        """The state scalars the REFERENCE graph creates for this config, in creation order (TensorFlow names unnamed variables
        `Variable`, `Variable_1`, ... by it): `loa` exists only under adversarial_regularization (model.py:886-890), `lor` only
        under variational_regularization (model.py:913-921); with one of them off the later names shift down."""
        skip = set()
        if not self.config.get("adversarial_regularization", True):
            skip.add("loa")
        if not self.config.get("variational_regularization", True):
            skip.add("lor")
        return tuple(k for k in self.TF_UNNAMED_ORDER if k not in skip)

    def _initialize_from_tf(self, prefix):
        """A TensorFlow-1.x checkpoint of the reference (``model.ckpt-<step>.index`` + ``.data-*``): variables are matched by
        name exactly as slim.assign_from_checkpoint(ignore_missing_vars=True) does (model.py:597-601), Adam slots
        (``<var>/Adam``, ``<var>/Adam_1``) are taken when present, the step comes from the file name."""
        from . import tfckpt
        import numpy as np
        bundle = tfckpt.read_bundle(prefix)
        params, m, v, _other = tfckpt.to_trainer_state(bundle)
        shadows = tfckpt.pop_shadows(_other)     # `<var>/ExponentialMovingAverage`: the weight EMA's shadows, not "unrestored scalars"
        keep = set(self.get_restore_variables())
        bank = self.model.bank
        loaded = {n: torch.from_numpy(np.ascontiguousarray(a)) for n, a in params.items()
                  if n in keep and n in bank.params and tuple(a.shape) == tuple(bank.params[n].shape)}
        bank.load(loaded)
        with torch.no_grad():
            for n in loaded:
                if n in m and n in v:
                    bank.adam_m[n].copy_(torch.from_numpy(np.ascontiguousarray(m[n])))
                    bank.adam_v[n].copy_(torch.from_numpy(np.ascontiguousarray(v[n])))
        digits = "".join(ch for ch in os.path.basename(prefix).split("-")[-1] if ch.isdigit())
        self.set_global_step(int(digits) if digits else 0)
        for key, grp in bank.groups.items():
            if any(n in loaded and n in m for n in grp["names"]):
                grp["t"] = self.global_step        # one Adam step per global step and key (beta powers are not stored per name)
        if self.logger:
            self.logger.info("Lazily restored {} of {} variables from the TensorFlow checkpoint {}".format(
                len(loaded), len(bank.params), prefix))
        # (a bundle carries no update counts: tf.train.ExponentialMovingAverage takes num_updates from the global step, and so does this)
        self._restore_ema({n: np.ascontiguousarray(a) for n, a in shadows.items()} or None, self.global_step, keep, prefix)
        self.restored_from_tf = sorted(loaded)
        # what slim.assign_from_checkpoint would ALSO have restored but cannot be matched here: the reference's unnamed
        # non-trainable scalars (Lagrangian multipliers, EMAs) and the optimizers' beta powers.  Say so instead of silently
        # restarting them (the multipliers / EMAs start from their yaml initial values, Adam's step count from the file name).
        # The reference's graph creates ten unnamed scalar tf.Variables (eight / nine with a regulariser off, tf_unnamed_order),
        # which TensorFlow names by creation order:
        # `Variable` = lon (define_graph, model.py:503), `Variable_1..5` = the EMAs of make_loss_ops in source order
        # (model.py:829-834: avg_acc0, avg_acc1, avg_acc_error, avg_loss_dis0, avg_loss_dis1), `_6`, `_7` = the EMAs of the two MI
        # constraints (model.py:862, 865), `_8` = loa (890), `_9` = lor (921).  A bundle that holds exactly these ten scalars is
        # mapped in that order (UNVERIFIED against a real checkpoint: the shipped ones are Git-LFS stubs); anything else is
        # reported below instead of guessed.
        order = self.tf_unnamed_order()
        unnamed = ["Variable"] + ["Variable_{}".format(i) for i in range(1, len(order))]
        found = [n for n in _other if n == "Variable" or n.startswith("Variable_")]
        self.state_from_tf = {}
        if sorted(found) == sorted(unnamed) and all(np.asarray(_other[n]).size == 1 for n in unnamed):
            for key, n in zip(order, unnamed):
                if key in self.state:
                    self.state[key].fill_(float(np.asarray(_other[n]).reshape(-1)[0]))
                    self.state_from_tf[key] = n
                _other.pop(n)
            if self.logger:
                self.logger.info("Lagrangian state restored from the checkpoint's unnamed variables by creation order: {}".format(
                    ", ".join("{}<-{}".format(k, v) for k, v in self.state_from_tf.items())))
        self.not_restored_from_tf = sorted(n for n in _other if n != "global_step")
        if self.not_restored_from_tf:
            msg = ("TensorFlow checkpoint {}: {} non-trainable / optimizer scalars are NOT restored (unnamed in the reference's graph: "
                   "{} ...): lon / loa / lor and the EMAs restart from their initial values, Adam's bias correction from step {}"
                   .format(prefix, len(self.not_restored_from_tf), ", ".join(self.not_restored_from_tf[:4]), self.global_step))
            if self.logger:
                self.logger.warning(msg)
            else:
                import sys
                sys.stderr.write("[WARNING] " + msg + "\n")

    def export_tf_checkpoint(self, prefix, weights="current"):
        """Write the trainable variables (+ Adam slots) as a TensorFlow tensor bundle the reference's graph can restore.  With the
        weight EMA on, every shadow goes in as `<var>/ExponentialMovingAverage` (tf.train.ExponentialMovingAverage's name);
        weights="ema" writes the shadows under the plain variable names as well, so that the reference's graph restores EMA weights."""
        from . import tfckpt
        import numpy as np
        if weights not in ("current", "ema"):
            raise ValueError("export_tf_checkpoint: weights is \"current\" or \"ema\" (got {!r})".format(weights))
        if weights == "ema" and self._ema is None:
            raise ValueError("export_tf_checkpoint(weights=\"ema\"): the weight EMA is off (ema_decay: 0)")
        bank = self.model.bank
        tensors = {}
        shadows = self.ema_state() if self._ema is not None else {}
        for n, t in shadows.items():
            tensors[n + tfckpt.EMA_SUFFIX] = t.numpy()
        for n, p in bank.params.items():
            tensors[n] = shadows[n].numpy() if weights == "ema" and n in shadows else p.detach().cpu().numpy()
            tensors[n + "/Adam"] = bank.adam_m[n].detach().cpu().numpy()
            tensors[n + "/Adam_1"] = bank.adam_v[n].detach().cpu().numpy()
        tensors["global_step"] = np.asarray(self.global_step, dtype=np.int64)
        # the Lagrangian state under the names TensorFlow gives the reference's ten unnamed scalar variables (creation order:
        # see _initialize_from_tf)
        for i, key in enumerate(self.tf_unnamed_order()):
            if key in self.state:
                tensors["Variable" if i == 0 else "Variable_{}".format(i)] = np.asarray(float(self.state[key]), dtype=np.float32)
        tfckpt.write_bundle(prefix, tensors)

    def save_checkpoint(self, path):
        if self._poisoned:
            raise RuntimeError("refusing to write a checkpoint: " + self._poisoned)
        bank = self.model.bank
        extra = {}
        if self._ema is not None:       # the shadows by variable name (`restore_exclude` applies to them as to params) and the keys' counts
            extra["ema"] = {"params": self.ema_state(), "n": dict(self.ema_report())}
        torch.save({"params": bank.state(), "global_step": self.global_step, **extra,
                    "adam": {k: {"m": g["flat"]["m"].cpu(), "v": g["flat"]["v"].cpu(), "t": g["t"]}
                             for k, g in bank.groups.items()},
                    "state": {k: float(v) for k, v in self.state.items()},
                    # a resumed run continues the sampling-noise stream instead of replaying steps 0..N's draws
                    "noise_offset": self._noise.offset, "gen_state": self._gen.get_state().cpu(),
                    "rank": self.rank, "world_size": self.world_size}, path)

    # ------------------------------------------------------------------ helpers
    def draw_noise(self, B):
        cfg = self.config
        S, P, Z = cfg["spatial_size"], self.model.n_parts, cfg.get("z0_size", 256)
        r = lambda *s: self._noise.randn(*s, device=self.device)      # the library's own Philox kernel (ops.NoiseStream)
        # (the mask noise of both views as ONE [2B,S,S,P] tensor: what part_softmax takes -- two tensors would be concatenated,
        # 168 MB of copies at B = 64; explicit noise may still come as eps_l0 / eps_l1, the fixtures' form)
        out = {"eps_pi0": r(9 if self.model.df else 7, B, Z), "eps_pi1": r(B, Z), "eps_l": r(2 * B, S, S, P)}
        if self.perceptual_input == "resize256_crop224":     # corner of the step's 224x224 window of the 256x256 images
            out["crop_yx"] = torch.randint(0, 33, (2,), generator=self._gen, device=self.device, dtype=torch.int32)
        return out

    def learning_rate(self):
        cfg = self.config
        lr = cfg.get("lr", 1e-4)
        lr = make_linear_var(self.global_step, cfg.get("lr_decay_begin", 1000), cfg.get("lr_decay_end", 1001), lr, 0.0,
                             0.0, lr)
        if self.lr_warmup_steps > 0:
            lr = lr * min(1.0, (self.global_step + 1.0) / self.lr_warmup_steps)
        return lr

    def _prior(self, view, n, S, P, l, lm, m, hard, px, per_np, sums, w, g_hard=None, dl=None, bwd=False, dl_rec=None):
        d = L.PriorDesc()
        d.n, d.h, d.w, d.P, d.view = n, S, S, P, view
        d.half_h = d.half_w = self.model.patch_size // 2
        if self.model.df:        # SB_model48c:719-776: CE labels always, no gamma, alpha / lambda from the yaml schedules
            d.variant, d.entropy_ce, d.gamma = 1, 1, 1.0
            d.ms_alpha = make_var(self.global_step, self.config["mumford_sha_alpha"])
            d.ms_lambda = make_var(self.global_step, self.config["mumford_sha_lambda"])
            d.w_ms_logits = w.get("msl", 0.0)
        else:
            d.variant = 0
            ef = self.config.get("entropy_func", "cross_entropy")
            if ef not in ("cross_entropy", "entropy"):
                raise ValueError("unkown entropy_func")               # model.py:680 (spelling as in the reference)
            d.entropy_ce = int(ef == "cross_entropy")
            d.gamma = float(self.config.get("gamma", 3.0))
            d.ms_alpha, d.ms_lambda = 1.0, 1.0e-2                  # hard-coded at model.py:744-746
        d.w_kl, d.w_entropy, d.w_ms, d.w_area = w["kl"], w["entropy"], w["ms"], w["area"]
        d.w_patch, d.w_gmrf, d.w_var = w["patch"], w["gmrf"], w["var"]
        g = lambda t: t.data_ptr() if t is not None else None
        d.l, d.l_mean, d.m, d.hard, d.px = g(l), g(lm), g(m), g(hard), g(px)
        d.per_np, d.sums, d.g_hard, d.dl = g(per_np), g(sums), g(g_hard), g(dl)
        d.dl_rec = g(dl_rec)
        L.call("ups_prior_bwd" if bwd else "ups_prior_fwd", C.byref(d), L.stream())

    # ------------------------------------------------------------------ one session.run(train_op)
    def train_step(self, batch, noise=None, images=False):
        """One session.run(train_op).  images=True: the step's image logs are rendered into ``img_ops`` as well (``_render_images``;
        ``iterate`` asks for them on the steps it logs scalars when the config sets ``log_images``).  With ``hip_graph: True`` the whole
        step -- ~1 000 kernel launches on three streams -- is captured once into HIP graphs and replayed (one graph on a single GPU;
        under data parallelism a sequence of graphs cut at the collectives): ``_graph_step`` / ``stepsync.StepGraph``.  The optimizer
        keys' hand-off is ``self.sync`` (``stepsync.GradSync``); a step that raises after some keys have stepped poisons the trainer."""
        ops.Fp8.activate(self.model.fp8)
        if self._poisoned:
            raise RuntimeError("this trainer's state is inconsistent: " + self._poisoned + " -- restore a checkpoint (Trainer.initialize)")
        self._release_images()
        self._want_images = bool(images)
        try:
            return self._train_step(batch, noise)
        except BaseException as e:
            self._after_failed_step(e)
            raise
        finally:
            self._want_images = False

    def _after_failed_step(self, exc):
        """A step that raises after some optimizer keys have already taken their Adam step on the weight-gradient stream
        (EARLY_ADAM) leaves those keys at step t + 1 and the others at t, with the converted weight copies stale.  Make the
        device state coherent (side streams joined, copies re-converted from whatever the masters now hold) and refuse further
        steps / checkpoints: the run has to restart from its last checkpoint."""
        done = self.sync.abort()
        if not done:
            return
        try:
            ops.Streams.join(self.device, names=("wgrad", "aux", "pre"))
            ops.weights_changed(self.model.nets.prep)
        except Exception:
            pass
        self._poisoned = ("a training step failed ({}: {}) after the optimizer keys {} had been updated while the others had not"
                          .format(type(exc).__name__, exc, done))

    def _train_step(self, batch, noise=None):
        if self._graph_enabled:
            # one device scalar carries Adam's bias-corrected step size: usable only while every trained key is at the same
            # Adam step (not after restoring a checkpoint whose keys were trained for different numbers of steps)
            ts = set(self.model.bank.groups[k]["t"] for k in self.loss_keys())
            if len(ts) <= 1:
                return self._graph_step(batch, noise)
        return self._step_impl(batch, noise)

    # ------------------------------------------------------------------ HIP-graph replay of the step
    def _schedule_signature(self):
        """Everything the captured launches bake in by value: the step's schedule constants."""
        cfg, step = self.config, self.global_step
        keys = ("prior_gmrf_weight", "prior_mumford_sha_weight", "variance_weight", "weakly_superv_loss_weight_p",
                "patch_loss_weight", "mumford_sha_alpha", "mumford_sha_lambda")
        sig = tuple(make_var(step, cfg[k]) for k in keys if k in cfg)
        return sig + (make_linear_var(step, **cfg["kl_weight"]), bool(cfg.get("pretrain", False)))

    def _graph_step(self, batch, noise):
        """Static input / noise buffers + a device scalar for Adam's step size; the graph is (re)captured after two eager
        steps and whenever a schedule constant changes (staircases move every few thousand steps).  The small-batch
        configs of the reference (batch 8: ~2 400 launches for 24 ms of GPU work) are launch-bound without it."""
        B, S = batch["view0"].shape[0], batch["view0"].shape[1]
        if self.graph is None or self.graph.shape != (B, S):     # the capture bakes in shapes and workspace pointers: start over
            self.graph = None                    # (the old buffers go before the new ones are made)
            self.graph = SS.StepGraph(self, B, S)
        g = self.graph
        for k, buf in g.inputs.items():
            buf.copy_(batch[k], non_blocking=True)
        if g.tps_u is not None:     # the TPS uniforms: drawn where the eager step draws them, BEFORE the window corner (one `_gen` stream)
            if noise is None or "tps_u" not in noise:
                g.tps_u.uniform_(0, 1, generator=self._gen)
            else:
                g.tps_u.copy_(noise["tps_u"], non_blocking=True)
        for k, buf in g.noise.items():
            if k == "crop_yx" and (noise is None or "crop_yx" not in noise):     # (explicit noise without a window corner: drawn as usual)
                buf.random_(0, 33, generator=self._gen)
            elif noise is None:
                self._noise.fill(buf)
            elif k == "eps_l" and "eps_l" not in noise:          # explicit noise in the fixtures' two-tensor form
                buf[:B].copy_(noise["eps_l0"], non_blocking=True)
                buf[B:].copy_(noise["eps_l1"], non_blocking=True)
            else:
                buf.copy_(noise[k], non_blocking=True)
        t = self.model.bank.groups[self.loss_keys()[0]]["t"] + 1
        lr = self.learning_rate()
        g.lr.fill_(lr * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t))
        sig = self._schedule_signature() + (lr > 0,)
        step_noise = g.noise if g.tps_u is None else dict(g.noise, tps_u=g.tps_u)
        run_step = lambda: self._step_impl(g.inputs, step_noise, graph_lr=g.lr)
        # warm-up: kernel attributes, side streams, allocator pools; fp8: the copy hand-off settles over four steps (first maxima,
        # first copies, unread producers going quiet) and the captured graph freezes whatever it sees
        if g.eager < (5 if ops.Fp8.enabled else 2):
            g.eager += 1
            out = run_step()
            self._after_graph_step()
            return out
        if not g.graphs or g.sig != sig:
            g.capture(run_step, sig)    # (capturing does not execute: the replay below runs the step)
        g.replay()
        self._after_graph_step()
        if self._want_images:           # outside the captured graphs, after the replay, from the buffers the capture owns
            self._render_images(g.img_src, self.global_step - 1)
        return _LazyLosses(self)

    def _after_graph_step(self):
        # (WeightVersion is not bumped: the step's own batched weight_prep has already refreshed every converted copy)
        for k in self.loss_keys():               # keys under `fix_weights` are not stepped (as in eager mode)
            self.model.bank.groups[k]["t"] += 1
        self.global_step += 1

    # ------------------------------------------------------------------ the step, segment by segment.  `c` (a _Step) carries the
    # step's tensors from one segment to the next; the order of the calls in _step_impl IS the order of the launches.
    def _step_begin(self, batch, noise):
        """Inputs (+ in-graph TPS, model.py:334-337), noise, schedule constants; starts the perceptual features of the TARGET on
        the "pre" stream (they depend on the data only and fill the bubbles of the small layers at the network ends)."""
        cfg, model, dev = self.config, self.model, self.device
        c = _Step()
        c.keys, c.step, c.df, c.T = self.loss_keys(), self.global_step, model.df, model.act_dtype
        df = c.df
        v0 = batch["view0"].to(dev, torch.float32).contiguous()
        v1 = batch["view1"].to(dev, torch.float32).contiguous()
        vt = v0 if df else batch["view0_target"].to(dev, torch.float32).contiguous()    # SB_model48c:669: target = view0
        if model.use_tps:           # model.py:334-337, 282-311
            tu = None if noise is None or "tps_u" not in noise else noise["tps_u"].to(dev, torch.float32)
            aug = TPS.make_tps([v0, v1] if df else [v0, v1, vt], model.tps_parameters, uniforms=tu, generator=self._gen,
                               n_singular=self._tps_singular)
            c.raw_views = (v0, v1, vt)          # the inputs as they came (img_ops view0 / view1 / view0_target)
            v0, v1 = aug[0], aug[1]
            vt = v0 if df else aug[2]
            model._tps = {"tps_view0": v0, "tps_view1": v1, "tps_view0_target": vt}
        c.v0, c.v1, c.vt = v0, v1, vt
        c.B, c.S = v0.shape[0], v0.shape[1]
        c.Z, c.A, c.P = cfg.get("z0_size", 256), cfg.get("local_app_size", 64), model.n_parts
        c.gamma = float(cfg.get("gamma", 3.0))
        c.half = model.patch_size // 2
        c.main_stream = torch.cuda.current_stream(dev)
        # `perceptual_input` (the three readings of edflow VGG19Features(original_scale=True), model.py:610-612, UNVERIFIED):
        # native | resize256 (128x128 inputs are up-sampled x2 with the legacy bilinear kernel, 256x256 inputs already have that
        # size) | resize256_crop224 (then ONE random 224x224 window for the whole batch, target and reconstruction alike;
        # its corner is the explicit noise input `crop_yx`, int32 [2] on the device)
        c.pmode = self.perceptual_input
        if c.pmode not in PERCEPTUAL_INPUTS:
            raise NotImplementedError("perceptual_input: {} ({})".format(c.pmode, " | ".join(PERCEPTUAL_INPUTS)))
        c.resize2x = False
        if c.pmode != "native":
            if c.S not in (128, 256):
                raise NotImplementedError("perceptual_input: {} is restated for 128x128 and 256x256 inputs only (got {})".format(c.pmode, c.S))
            c.resize2x = c.S == 128
        if noise is None:
            noise = self.draw_noise(c.B)
        c.crop_yx = None
        if c.pmode == "resize256_crop224":
            if df:
                raise NotImplementedError("perceptual_input: resize256_crop224 is restated for the SB_model48i variants only")
            if "crop_yx" not in noise:          # explicit (fixture-style) noise without a window corner: draw it as usual
                noise = dict(noise, crop_yx=torch.randint(0, 33, (2,), generator=self._gen, device=dev, dtype=torch.int32))
            c.crop_yx = noise["crop_yx"].to(dev, torch.int32).contiguous()
        c.ft_pre, c.ft_ready = None, None
        if ops.Streams.enabled:
            pre = ops.Streams.get("pre", dev)
            # (Letting this block start before the previous step's tail -- it depends on the batch alone -- measured neutral twice,
            # UPS_PRE_FREE in round 5: docs/design/negative_results.md; retired in round 6.)
            pre.wait_stream(c.main_stream)
            with torch.cuda.stream(pre), torch.no_grad():
                tgt_pre = vt if c.pmode == "native" else self._perceptual_view(c, model.to_act(vt))
                c.ft_pre = self.vgg.features(tgt_pre, c.T)
            c.ft_ready = pre.record_event()
        c.noise = {k: v.to(dev, torch.float32).contiguous() for k, v in noise.items() if k != "crop_yx"}
        c.st = self.state
        # ---- schedule constants of this step (model.py:621-646, 709-726, 774-779)
        step = c.step
        c.w_gmrf = make_var(step, cfg["prior_gmrf_weight"])
        c.w_ms = make_var(step, cfg["prior_mumford_sha_weight"])
        c.w_kl = make_linear_var(step, **cfg["kl_weight"])
        c.w_var = make_var(step, cfg["variance_weight"])
        c.w_weak = make_var(step, cfg["weakly_superv_loss_weight_p"])
        c.w_patch = 0.0 if df else make_var(step, cfg["patch_loss_weight"])
        c.pretrain = bool(cfg.get("pretrain", False))
        mi = cfg["MI"]
        c.mi, c.MI_TARGET, c.MI_SLACK = mi, mi.get("mi_target", 0.125), mi.get("mi_slack", 0.05)
        c.beta_0 = cfg.get("beta_0", 1.0)
        c.var_reg = cfg.get("variational_regularization", True)
        return c

    def _perceptual_view(self, c, x_act):
        """What the perceptual trunk sees of an image in the activation layout [n,S,S,8] (`perceptual_input`)."""
        if c.resize2x:
            x_act = ops.BilinearFn.apply(x_act)
        if c.crop_yx is not None:
            x_act = ops.CropFn.apply(x_act, c.crop_yx, 224, 224)
        return x_act

    def _fwd_pose(self, c):
        """A forward: pose encoder + full-covariance latent (model.py:382-409); nine / seven draws of z_0, one of z_1."""
        model, nets = self.model, self.model.nets
        B, S = c.B, c.S
        c.img01 = torch.empty((2 * B, S, S, 8), dtype=c.T, device=self.device)     # both views, each converted into its half
        model.to_act(c.v0, out=c.img01[:B])
        model.to_act(c.v1, out=c.img01[B:])
        if EARLY_ALPHA:
            self._alpha(c)
        c.pe = nets.e_pi(Act(c.img01, 2 * B, S, S, 3)).t                  # fp32 [2B,1,1,NP], taped
        c.pe2 = c.pe.detach().view(2 * B, -1)
        c.pe_v0, c.pe_v1 = c.pe2[:B].contiguous(), c.pe2[B:].contiguous()
        lon = 1.0                                                         # LON_ADAPTIVE = False (model.py:842): lon stays 1
        c.levels0 = [1.0, lon, lon, 1.0, 1.0, 1.0, 1.0]                   # draw order model.py:406,506,509,512,514,518,520
        if c.df:
            c.levels0 += [1.0, 1.0]                                       # SB_model48c:492,502: two more draws of z_00
        c.samples0, c.kl_rows = ops.latent_fwd(c.pe_v0, c.noise["eps_pi0"], c.levels0, True)
        c.samples1, _ = ops.latent_fwd(c.pe_v1, c.noise["eps_pi1"][None], [1.0], False)

    def _alpha(self, c):
        """Appearance code of the whole views: it feeds the critics only -> forward only (model.py:394-397).  It depends on the
        images alone, so it is enqueued on the "aux" stream BEFORE the pose encoder goes to the launching stream: the two encoders
        run side by side, and the critics can start the moment the latent samples exist."""
        nets, B, S = self.model.nets, c.B, c.S

        def run():
            with torch.no_grad():
                c.alpha = nets.e_alpha(Act(c.img01, 2 * B, S, S, 3)).t            # [2B,1,1,A]
                c.alpha_in = torch.cat([c.alpha[B:], torch.flip(c.alpha[:B], dims=[0])], 0).contiguous()
        if ops.Streams.enabled:
            aux = ops.Streams.get("aux", self.device)
            aux.wait_stream(c.main_stream)
            with torch.cuda.stream(aux):
                run()
        else:
            run()

    def _critics(self, c, forked_at=None):
        """D: the three critics (model.py:502-521, 800-866), their own gradients, the adversarial gradient d adv / d z_joint0 for
        encoder_0 (model.py:886-909) and, for SB_model48c, the three single-sample decoders.  They depend on the latent samples
        and on the appearance code of the whole views only, and the main path needs them again at the encoder_0 backward: the
        whole block (72 tiny GEMMs that cannot fill the chip) runs on the "aux" stream beside segments B and C."""
        cfg, model, nets, bank = self.config, self.model, self.model.nets, self.model.bank
        B, S, Z, A, keys, st, mi = c.B, c.S, c.Z, c.A, c.keys, c.st, c.mi
        if not EARLY_ALPHA:
            with torch.no_grad():
                c.alpha = nets.e_alpha(Act(c.img01, 2 * B, S, S, 3)).t            # [2B,1,1,A]
                c.alpha_in = torch.cat([c.alpha[B:], torch.flip(c.alpha[:B], dims=[0])], 0).contiguous()
        alpha, alpha_in = c.alpha, c.alpha_in
        crit = {}
        c.adv, c.g_adv = None, None
        names = ("mi0_discriminator", "mi1_discriminator", "mi_estimator")

        def one(ci, name):
            pi_in = model.to_act(torch.cat([c.samples0[1 + 2 * ci], c.samples0[2 + 2 * ci]], 0).view(2 * B, 1, 1, Z))
            pi_in.requires_grad_(name == "mi0_discriminator")
            h_pi, h_al = nets.critic(name, (Act(pi_in, 2 * B, 1, 1, Z), Act(alpha_in, 2 * B, 1, 1, A)))
            # dot product of the two embeddings, logistic losses, accuracy and the mean joint logit: one launch (+ one backward)
            loss, acc, mean_joint = ops.CriticHeadFn.apply(h_pi.t, h_al.t, B, N.DSIZE)
            crit[name] = (loss, mean_joint, acc, pi_in)
            if ci == 0:
                c.mim = mean_joint                                            # logit_constraint(real=False), model.py:855
                if cfg.get("adversarial_regularization", True):               # model.py:886-909
                    loa, loa_lr = st["loa"], mi.get("loa_lr", 4.0)
                    loa_gain = c.mim - (1.0 - c.MI_SLACK) * c.MI_TARGET
                    if mi.get("loa_adaptive", True):
                        active = (loa_lr * loa_gain.detach() >= -loa).float()
                        c.adv = active * (loa * loa_gain + loa_lr / 2.0 * loa_gain ** 2)
                    else:
                        c.adv = loa * loa_gain
                    if "encoder_0" in keys:
                        with ops.skip_wgrad():
                            c.g_adv = torch.autograd.grad([c.adv], [pi_in], retain_graph=True)[0].float().view(2 * B, Z)[:B]
            elif ci == 1:
                c.ind_mim = mean_joint
            if name in keys:
                torch.autograd.grad([loss], [bank.params[n] for n in bank.groups[name]["names"]])

        # the three critics are independent chains of ~80 launches of a few blocks each; behind a main stream whose kernels fill
        # every CU each of those launches waits for a slot, so the chains run side by side on three streams (all joined into "aux")
        cur = torch.cuda.current_stream(self.device)
        # (not in a captured step: replayed from a HIP graph the three branches cost more than they save -- 1 887 against 1 919 img/s
        # with one critic stream, eager 1 979 -- so a capture keeps the one-stream form)
        multi = ops.Streams.enabled and ops.Streams.on_aux(self.device) and CRITIC_STREAMS and c.graph_lr is None
        # (the two extra critic streams stay created even when the critics run as grouped launches: which streams share a hardware
        # queue depends on the creation order, and the order without them sits in the slower cluster -- docs/design/negative_results.md)
        sides = [cur] + ([ops.Streams.get("aux{}".format(i), self.device) for i in (1, 2)] if multi else [cur, cur])
        for sd in sides[1:]:
            if sd is not cur:
                if forked_at is not None:          # (the launching stream has moved on to the mask decoder: fork where the samples exist)
                    sd.wait_event(forked_at)
                else:
                    sd.wait_stream(c.main_stream)  # forked from the launching stream (a HIP-graph capture wants first-level forks) ...
                sd.wait_stream(cur)                # ... and behind the appearance code
        if not self._critics_grouped(c, names, crit, alpha_in):
            for ci, name in enumerate(names):
                with torch.cuda.stream(sides[ci]):
                    one(ci, name)
        if c.df:
            # SB_model48c:491-505, 672-684, 812-814: three single-sample decoders on batch item 0 (inputs under
            # stop_gradient), each with its own perceptual loss and optimizer key; one per side stream, behind that stream's critic
            scale = 1e-3 * 0.5 * (S * S * 3)

            def a1():
                return alpha[B:B + 1, ..., :A].float().reshape(1, A)
            ins = {"d_single": (lambda: torch.cat([c.samples0[7][:1], a1()], 1), c.v0[:1], Z + A),
                   "d_alpha": (a1, c.v1[:1], A), "d_pi": (lambda: c.samples0[8][:1], c.v0[:1], Z)}
            for i, (name, (zin, tgt, cz)) in enumerate(ins.items()):
                with torch.cuda.stream(sides[i]):
                    g_img = nets.dsingle(name, Act(model.to_act(zin().view(1, 1, 1, cz)), 1, 1, 1, cz)).t
                    lss = scale * self.vgg.loss(tgt.contiguous(), g_img, c.T, gram_weight=self.gram_weight)
                    crit[name] = (lss, g_img)
                    if name in keys:
                        torch.autograd.grad([lss], [bank.params[n] for n in bank.groups[name]["names"]])
        # ("aux1" / "aux2" are joined wherever "aux" is: ops.Streams.join)
        c.crit = crit
        c.loss_dis0, _, c.acc0, _ = crit["mi0_discriminator"]
        c.loss_dis1, _, c.acc1, _ = crit["mi1_discriminator"]
        c.loss_est, _, c.acc_est, _ = crit["mi_estimator"]

    def _critics_grouped(self, c, names, crit, alpha_in):
        """The three critics through ops.TowersFn (round 5): six towers of six 1x1 layers as 6 forward launches, 5 + 1 input-gradient
        launches per backward call and ONE launch for all 72 weight / bias gradients, on the current ("aux") stream -- against ~210
        launches of a few blocks each on three streams.  The same graph as `one` above: the adversarial term differentiates critic
        0's pi tower alone (skip_wgrad, retain_graph), the critics' own losses are differentiated together (their variables are
        disjoint, so the sum's gradient is each loss's).  Returns False when the towers do not have the form the grouped launches
        take (fp32 / non-leaky / materialised storage): the caller then runs the generic path."""
        cfg, model, nets, bank = self.config, self.model, self.model.nets, self.model.bank
        B, Z, A, keys, st, mi = c.B, c.Z, c.A, c.keys, c.st, c.mi
        if not ops.TOWERS:
            return False
        towers = []
        for name in names:
            tw = nets.critic_layers(name, (Z, A))
            if tw is None:
                return False
            towers += tw
        pi_ins = [model.to_act(torch.cat([c.samples0[1 + 2 * ci], c.samples0[2 + 2 * ci]], 0).view(2 * B, 1, 1, Z)) for ci in range(3)]
        xs = [x for ci in range(3) for x in (pi_ins[ci], alpha_in)]
        if not ops.towers_eligible(towers, xs) or Z % 128 or pi_ins[0].shape[-1] != Z:      # (the adversarial term's input gradient is
            return False                                                                    # written 128 channels per block)
        pi_ins[0].requires_grad_(True)
        params = [t for tw in towers for lay in tw for t in (lay.V, lay.b)]
        hs = ops.TowersFn.apply(towers, *(xs + params))
        losses = []
        for ci, name in enumerate(names):
            loss, acc, mean_joint = ops.CriticHeadFn.apply(hs[2 * ci], hs[2 * ci + 1], B, N.DSIZE)
            crit[name] = (loss, mean_joint, acc, pi_ins[ci])
            if ci == 0:
                c.mim = mean_joint                                            # logit_constraint(real=False), model.py:855
                if cfg.get("adversarial_regularization", True):               # model.py:886-909
                    loa, loa_lr = st["loa"], mi.get("loa_lr", 4.0)
                    loa_gain = c.mim - (1.0 - c.MI_SLACK) * c.MI_TARGET
                    if mi.get("loa_adaptive", True):
                        active = (loa_lr * loa_gain.detach() >= -loa).float()
                        c.adv = active * (loa * loa_gain + loa_lr / 2.0 * loa_gain ** 2)
                    else:
                        c.adv = loa * loa_gain
                    if "encoder_0" in keys:
                        with ops.skip_wgrad():
                            c.g_adv = torch.autograd.grad([c.adv], [pi_ins[0]], retain_graph=True)[0].float().view(2 * B, Z)[:B]
            elif ci == 1:
                c.ind_mim = mean_joint
            if name in keys:
                losses.append((name, loss))
        if losses:
            torch.autograd.grad([l for _, l in losses], [bank.params[n] for name, _ in losses for n in bank.groups[name]["names"]])
        return True

    def _fwd_masks(self, c):
        """B forward: mask decoder z -> logits (model.py:411-412), then the un-taped part path (model.py:414-473): l = mean + eps,
        soft-max, hard max, the moments of gamma * hard and the rectangle centres."""
        cfg, model, nets = self.config, self.model, self.model.nets
        B, S, P = c.B, c.S, c.P
        z_act = model.latent_act(torch.cat([c.samples0[0], c.samples1[0]], 0))
        c.z_leaf = z_act.t.requires_grad_(True)
        c.l_mean = nets.dv(z_act).t                                       # fp32 [2B,S,S,P], taped
        c.lm = c.l_mean.detach()
        # model.py:420-421 / nn.py:1427-1433: l = mean + eps unless `stochastic_l: False` (default: not test_mode)
        stochastic_l = cfg.get("stochastic_l", not cfg.get("test_mode", False))
        eps_l = None
        if stochastic_l:
            eps_l = c.noise["eps_l"] if "eps_l" in c.noise else torch.cat([c.noise["eps_l0"], c.noise["eps_l1"]], 0)
        # (the moments of gamma * hard -- the input of the rectangle centres, model.py:437-440 -- come out of the same pass)
        if c.df:
            c.l, c.m, c.hard, _, c.hbits = ops.part_softmax(c.lm, eps_l, want_bits=P <= 32)
            hstats = None
        else:
            c.l, c.m, c.hard, _, c.hbits, hstats = ops.part_softmax(c.lm, eps_l, want_bits=P <= 32, moments_gamma=c.gamma)
        # [2B,P,2] rectangle centres (stop-gradient); SB_model48c has no rectangles
        if c.df:
            c.px = None
        else:
            if hstats is None:
                hstats = ops.spatial_moments(c.hard, c.gamma)
            c.px = ops.moments_to_px(hstats, S, cfg.get("rect_order", "xy"))
        c.hard0 = c.hard[:B].detach().requires_grad_(True)
        c.hard1 = c.hard[B:].detach().requires_grad_(True)

    def _fwd_reconstruction(self, c):
        """C forward: part-wise appearance -> unpool -> image decoder -> perceptual loss (model.py:478-485, 607-619)."""
        model, nets = self.model, self.model.nets
        B, S, A, P, T = c.B, c.S, c.A, c.P, c.T
        parts = model.part_images(c.img01[B:], c.v1, c.hard1, None if c.hbits is None else c.hbits[B:].contiguous())
        yp = nets.e_alpha(parts).t                                         # [P*B,1,1,A]
        c.feat = yp.float().view(P, B, A).permute(1, 0, 2).contiguous()    # [B,P,A]
        inj = ops.UnpoolFn.apply(c.hard0, c.feat, T)
        c.gen = nets.dd(Act(inj, B, S, S, A + P)).t                        # [B,S,S,8]
        gen_in = self._perceptual_view(c, c.gen)
        if c.ft_pre is not None:
            c.main_stream.wait_event(c.ft_ready)
            c.rec = self.vgg.loss(None, gen_in, T, target_features=c.ft_pre, gram_weight=self.gram_weight)
        else:
            tgt_in = c.vt if c.pmode == "native" else self._perceptual_view(c, model.to_act(c.vt))
            c.rec = self.vgg.loss(tgt_in, gen_in, T, gram_weight=self.gram_weight)
        c.auto_rec = (1e-3 * 0.5 * (S * S * 3)) * c.rec                    # model.py:613-619

    def _bwd_reconstruction(self, c):
        """C backward: encoder_1 / decoder_delta weight gradients (they land in the flat buckets) and d rec / d hard masks."""
        bank = self.model.bank
        rec_keys = [k for k in ("encoder_1", "decoder_delta") if k in c.keys]
        rec_params = [bank.params[n] for k in rec_keys for n in bank.groups[k]["names"]]
        gr = torch.autograd.grad([c.auto_rec], [c.hard0, c.hard1] + rec_params)
        c.g_hard0, c.g_hard1 = gr[0].contiguous(), gr[1].contiguous()
        self.sync.segment_done(rec_keys)

    def _priors(self, c):
        """Mask priors: fused forward sums + fused analytic backward (model.py:652-797).  One backward launch per view emits both
        d(rec + priors)/dl (what the decoder_visualize key sees) and d(rec)/dl (what encoder_0 sees)."""
        dev = self.device
        B, S, P, df = c.B, c.S, c.P, c.df
        nfl = L.load().ups_prior_sums_floats(B, P)
        c.sums0 = torch.empty(nfl, dtype=torch.float32, device=dev)
        c.sums1 = torch.empty(nfl, dtype=torch.float32, device=dev)
        per_np0 = torch.empty((B, P, 8), dtype=torch.float32, device=dev)
        l0, l1, m0, m1 = c.l[:B], c.l[B:], c.m[:B], c.m[B:]
        px0, px1 = (None, None) if df else (c.px[:B].contiguous(), c.px[B:].contiguous())
        wz = {"kl": 0.0, "entropy": 0.0, "ms": 0.0, "area": 0.0, "patch": 0.0, "gmrf": 0.0, "var": 0.0, "msl": 0.0}
        if c.pretrain:
            wp = dict(wz)
        elif df:     # SB_model48c:830-838
            wp = {"kl": c.w_kl, "entropy": c.w_weak, "ms": 0.0, "area": 0.0, "patch": 0.0, "gmrf": c.w_gmrf, "var": c.w_var, "msl": c.w_ms}
        else:
            wp = {"kl": c.w_kl, "entropy": c.w_weak, "ms": c.w_ms, "area": 1.0e-12, "patch": c.w_patch, "gmrf": c.w_gmrf, "var": c.w_var,
                  "msl": 0.0}
        self._prior(0, B, S, P, l0, c.lm[:B], m0, c.hard[:B], px0, per_np0, c.sums0, wp)
        # view 1: variance moments (model.py:683-707; SB_model48c:750-756: no gamma, no rectangle) and, from the same pass over the
        # map, its categorical KL (sums1[0]) -- the separate forward launch of view 1 is gone
        c.stats_v = ops.spatial_moments(m1.contiguous(), 1.0 if df else c.gamma, rect_px=px1, half=c.half, kl_sums=c.sums1)
        c.dl_tot = torch.empty_like(c.lm)
        c.dl_rec = torch.empty_like(c.lm)
        self._prior(0, B, S, P, l0, c.lm[:B], m0, c.hard[:B], px0, per_np0, c.sums0, wp, c.g_hard0, c.dl_tot[:B], bwd=True,
                    dl_rec=c.dl_rec[:B])
        self._prior(1, B, S, P, l1, None, m1, None, px1, c.stats_v, c.sums1, wp, c.g_hard1, c.dl_tot[B:], bwd=True, dl_rec=c.dl_rec[B:])
        rs = self.probe.get("rec_scale")
        if rs is not None and float(rs) != 1.0:     # diagnostic hook: how strongly the mask decoder's update follows the reconstruction term
            c.dl_tot.copy_((c.dl_tot - c.dl_rec) + float(rs) * c.dl_rec)

    def _bwd_mask_decoder(self, c):
        """B backward: the weights see rec + priors, the latent sees rec only (one extra input-gradient pass)."""
        bank = self.model.bank
        if "decoder_visualize" in c.keys:
            dv_params = [bank.params[n] for n in bank.groups["decoder_visualize"]["names"]]
            torch.autograd.grad([c.l_mean], dv_params, grad_outputs=[c.dl_tot], retain_graph=True)
        self.sync.segment_done([k for k in ("decoder_visualize",) if k in c.keys])
        with ops.skip_wgrad():
            c.gz = torch.autograd.grad([c.l_mean], [c.z_leaf], grad_outputs=[c.dl_rec])[0].float().view(2 * c.B, c.Z)

    def _bwd_pose(self, c):
        """A backward (model.py:739, 909, 930): d rec / d z (from B), the adversarial gradient on the joint sample of mi0 and the
        bottleneck beta_0 * exp(lor) * KL."""
        dev, bank = self.device, self.model.bank
        B, Z = c.B, c.Z
        if c.var_reg:
            assert not self.config.get("test_mode", False)
            explor = torch.exp(c.st["lor"])
        if "encoder_0" not in c.keys:
            return
        g_s0 = torch.zeros((len(c.levels0), B, Z), dtype=torch.float32, device=dev)
        g_s0[0] = c.gz[:B]
        if c.g_adv is not None:
            g_s0[1] = c.g_adv
        gp0 = ops.latent_bwd(c.pe_v0, c.noise["eps_pi0"], c.levels0, g_s0, explor.reshape(1) if c.var_reg else None,
                             c.beta_0 / B if c.var_reg else 0.0)
        gp1 = ops.latent_bwd(c.pe_v1, c.noise["eps_pi1"][None], [1.0], c.gz[B:].contiguous()[None], None, 0.0)
        g_pe = torch.cat([gp0, gp1], 0).view_as(c.pe)
        e0_params = [bank.params[n] for n in bank.groups["encoder_0"]["names"]]
        self.sync.hook_head()           # (data parallel, once: the head's slice of the bucket starts its all-reduce from inside the backward pass)
        torch.autograd.grad([c.pe], e0_params, grad_outputs=[g_pe])

    def _next_state(self, c):
        """update_ops (model.py:28-35, 829-834, 861-866, 890-909, 921-930): EMAs and the two multipliers from the batch-mean
        scalars -- averaged over the ranks first, so that every replica holds the same state.  Appendix A.15: the losses of this
        step used the pre-update state."""
        cfg, st, mi = self.config, c.st, c.mi
        stats = torch.stack([c.mim.detach(), c.ind_mim.detach(), c.acc0, c.acc1, c.loss_dis0.detach(), c.loss_dis1.detach()])
        if self.graph is not None and self.graph.capturing and self.world_size > 1:
            self.graph.boundary("scalars", stats)             # (the tensor lives in the graphs' pool: same address at every replay)
        else:
            D.average_scalars(stats, self.world_size, self.process_group)
        new = dict(st)
        up_loa = bool(cfg.get("adversarial_regularization", True) and mi.get("loa_adaptive", True))
        up_lor = bool(c.var_reg and mi.get("lor_adaptive", True))
        if (STATE_KERNEL or self.skip_nonfinite) and stats.is_cuda and all(st[k].dtype == torch.float32 and st[k].device == stats.device for k in STATE_KEYS):
            # one launch instead of ~30 scalar ones (they were the last thing a step enqueued, behind a drained GPU)
            old = torch.stack([st[k].reshape(()) for k in STATE_KEYS])
            vec = torch.empty_like(old)
            args = (0.99, 1.0 - 0.99, int(up_loa), mi.get("loa_lr", 4.0), (1.0 - c.MI_SLACK) * c.MI_TARGET, int(up_lor),
                    mi.get("lor_lr", 0.05), c.MI_TARGET, mi.get("lor_min", 1.0), mi.get("lor_max", 7.5))
            if self.skip_nonfinite:     # guarded by its own stats: a non-finite statistic leaves every EMA and both multipliers as they were
                ops.state_update_guarded(stats, old, vec, *args, self._guard_state)
            else:
                L.call("ups_state_update", L.ptr(stats), L.ptr(old), L.ptr(vec), *args, L.stream())
            for i, k in enumerate(STATE_KEYS):
                if k not in ("loa", "lor") or (k == "loa" and up_loa) or (k == "lor" and up_lor):
                    new[k] = vec[i]
            return new
        g_mim, g_ind, g_acc0, g_acc1, g_l0, g_l1 = stats.unbind(0)
        ema = lambda old, val: 0.99 * old + (1.0 - 0.99) * val            # model.py:28-35
        new["avg_acc0"] = ema(st["avg_acc0"], g_acc0); new["avg_acc1"] = ema(st["avg_acc1"], g_acc1)
        new["avg_acc_error"] = ema(st["avg_acc_error"], g_acc1 - g_acc0)
        new["avg_loss_dis0"] = ema(st["avg_loss_dis0"], g_l0); new["avg_loss_dis1"] = ema(st["avg_loss_dis1"], g_l1)
        new["avg_mim"] = ema(st["avg_mim"], g_mim); new["avg_independent_mim"] = ema(st["avg_independent_mim"], g_ind)
        if cfg.get("adversarial_regularization", True) and mi.get("loa_adaptive", True):
            new["loa"] = torch.clamp(st["loa"] + mi.get("loa_lr", 4.0) * (g_mim - (1.0 - c.MI_SLACK) * c.MI_TARGET), min=0.0)
        if c.var_reg and mi.get("lor_adaptive", True):
            new["lor"] = torch.clamp(st["lor"] + mi.get("lor_lr", 0.05) * (g_ind - c.MI_TARGET), mi.get("lor_min", 1.0),
                                     mi.get("lor_max", 7.5))
        return new

    def _log_thunk(self, c):
        """Losses per key + log ops (model.py:648-966; same names as the reference).  REPORTING only: ~150 scalar launches that no
        gradient depends on (the per-key gradients were taken from the pieces above).  In the eager trainer the returned closure is
        evaluated when somebody reads `losses` / `log_ops` (log steps, tests) and keeps only detached scalars and the small
        reduction buffers alive; inside a captured HIP graph it runs with the step."""
        cfg, st = self.config, c.st
        B, S, P, df, keys, step = c.B, c.S, c.P, c.df, c.keys, c.step
        w_gmrf, w_ms, w_kl, w_var, w_weak, w_patch, pretrain = c.w_gmrf, c.w_ms, c.w_kl, c.w_var, c.w_weak, c.w_patch, c.pretrain
        beta_0, var_reg, MI_TARGET, MI_SLACK = c.beta_0, c.var_reg, c.MI_TARGET, c.MI_SLACK
        sums0, sums1, stats_v, kl_rows = c.sums0, c.sums1, c.stats_v, c.kl_rows
        auto_rec, rec = c.auto_rec.detach(), c.rec.detach()
        adv = c.adv.detach() if c.adv is not None else None
        loss_dis0, loss_dis1, loss_est = c.loss_dis0.detach(), c.loss_dis1.detach(), c.loss_est.detach()
        acc0, acc1, acc_est = c.acc0, c.acc1, c.acc_est
        mim, ind_mim = c.mim.detach(), c.ind_mim.detach()
        crit_d = {k: c.crit[k][0].detach() for k in N.EXTRA_48C} if df else {}
        lr_now = self.learning_rate()          # (of THIS step: the counters have moved on when the logs are read)
        log = OrderedDict()

        def build_logs():
            bottleneck = kl_rows.sum(dim=1).mean()                            # nn.py:1196-1208
            bw = beta_0 * torch.exp(st["lor"]) * bottleneck if var_reg else None
            npx = float(B * S * S)
            prior_gmrf = sums0[3] / B
            mask0_kl = (sums0[0] + sums1[0]) / npx
            weakly = sums0[1] / npx
            patch_loss = sums0[2] / B
            p_ms = w_ms * sums0[4] / B
            area_cost = 1.0e-12 * sums0[5] / B
            Zs = stats_v[..., 1]
            if df:       # SB_model48c:757-776: squared diagonal variances of the (already normalised) maps
                s00 = stats_v[..., 6] / Zs - (stats_v[..., 3] / Zs) ** 2
                s11 = (stats_v[..., 5] - stats_v[..., 6]) / Zs - (stats_v[..., 4] / Zs) ** 2
                variances = (s00 ** 2 + s11 ** 2).sum(dim=1).mean()
                prior_ms = sums0[2] / B                                   # variant 1: the patch slot holds sum min(alpha g, lambda)
                prior_total = w_gmrf * prior_gmrf + prior_ms * w_ms + w_kl * mask0_kl + weakly * w_weak + w_var * variances
            else:
                variances = (stats_v[..., 5] / Zs - (stats_v[..., 3] / Zs) ** 2 - (stats_v[..., 4] / Zs) ** 2).sum(dim=1).mean()
                prior_total = (w_gmrf * prior_gmrf + w_kl * mask0_kl + weakly * w_weak + w_var * variances + p_ms + area_cost
                               + patch_loss * w_patch)

            Ls = OrderedDict()
            Ls["encoder_0"] = auto_rec + (adv if adv is not None else 0.0) + (bw if bw is not None else 0.0)
            Ls["encoder_1"] = auto_rec
            Ls["decoder_delta"] = auto_rec
            Ls["decoder_visualize"] = auto_rec if pretrain else auto_rec + prior_total
            Ls["mi0_discriminator"], Ls["mi1_discriminator"], Ls["mi_estimator"] = loss_dis0, loss_dis1, loss_est
            if df:       # SB_model48c:809-815 (the global term has no gradient path to the encoders: stop_gradient inputs)
                Ls["encoder_0"] = Ls["encoder_0"] + crit_d["d_single"]
                Ls["encoder_1"] = Ls["encoder_1"] + crit_d["d_single"]
                for k in N.EXTRA_48C:
                    Ls[k] = crit_d[k]
            losses_d = OrderedDict((k, Ls[k].detach()) for k in keys)
            avg_mim = torch.clamp(st["avg_mim"], min=0.0); avg_ind = torch.clamp(st["avg_independent_mim"], min=0.0)
            loo = torch.clamp((avg_ind - avg_mim) / (avg_ind + 1e-6), 0.0, 1.0)
            log.update({"prior_gmrf": prior_gmrf, "prior_gmrf_weight": w_gmrf, "prior_gmrf_weighted": w_gmrf * prior_gmrf,
                        "mask0_kl_weight": w_kl, "mask0_kl": mask0_kl, "mask0_kl_weighted": w_kl * mask0_kl,
                        "variance_loss_weighted": w_var * variances, "variance_loss": variances, "variance_weight": w_var,
                        "weakly_superv_loss_weight_p": w_weak, "weakly_superv_loss_p": weakly,
                        "weakly_superv_loss_p_weighted": weakly * w_weak,
                        "patch_loss": patch_loss, "patch_loss_weight": w_patch, "patch_loss_weighted": patch_loss * w_patch,
                        "mumford_sha_lambda": make_var(step, cfg["mumford_sha_lambda"]),
                        "mumford_sha_alpha": make_var(step, cfg["mumford_sha_alpha"]),
                        "avg_acc_error": st["avg_acc_error"], "avg_mim": avg_mim, "avg_independent_mim": avg_ind,
                        "loo": loo, "lon_gain": -loo + 0.025, "model_lon": st["lon"]})
            if df:
                for k in ("patch_loss", "patch_loss_weight", "patch_loss_weighted"):
                    log.pop(k)
            for k in Ls:
                log["loss_" + k] = Ls[k].detach()
            log.update({"dis0_accuracy": acc0, "dis1_accuracy": acc1, "avg_dis0_accuracy": st["avg_acc0"],
                        "avg_dis1_accuracy": st["avg_acc1"], "avg_loss_dis0": st["avg_loss_dis0"],
                        "avg_loss_dis1": st["avg_loss_dis1"], "est_accuracy": acc_est,
                        "mi_constraint": mim, "independent_mi_constraint": ind_mim})
            if adv is not None:
                log.update({"adversarial_weight": st["loa"], "adversarial_constraint": mim,
                            "adversarial_weighted_loss": adv, "loa": st["loa"],
                            "loa_gain": mim - (1.0 - MI_SLACK) * MI_TARGET})
            if bw is not None:
                log.update({"bottleneck_weight": st["lor"], "bottleneck_loss": bottleneck, "bottleneck_weighted_loss": bw,
                            "lor": st["lor"], "explor": beta_0 * torch.exp(st["lor"]), "lor_gain": ind_mim - MI_TARGET})
            if df:
                log.update({"prior_mumford_sha": prior_ms, "prior_mumford_sha_weight": w_ms, "prior_mumford_sha_weighted": prior_ms * w_ms,
                            "perceptual": rec, "lr": lr_now})
                for i in range(P):
                    log["sigma1_{:02d}".format(i)] = s00[0, i]
                    log["sigma2_{:02d}".format(i)] = s11[0, i]
            else:
                log.update({"zr_mumford_sha": p_ms, "z_mumford_sha_smoothness_cost": sums0[6] / B,
                            "z_mumford_sha_contour_cost": sums0[7] / B, "z_area_cost": area_cost,
                            "prior_mumford_sha_weight": w_ms, "perceptual": rec, "lr": lr_now})
            return losses_d, log
        return build_logs

    def _step_impl(self, batch, noise=None, graph_lr=None):
        """One training step on the launching stream (+ the "pre", "aux" and "wgrad" side streams): forward A -> D (aux) -> B ->
        C, backward C -> priors -> B -> A, each optimizer key's bucket reduced as soon as its segment is complete, Adam, state."""
        dev = self.device
        self.sync.begin(graph_lr)
        c = self._step_begin(batch, noise)
        c.graph_lr = graph_lr
        self._fwd_pose(c)
        # (enqueueing the mask decoder's forward pass BEFORE the critics' block measured neutral twice, UPS_CRITICS_LATE in round 5:
        # retired in round 6)
        if ops.Streams.enabled:
            aux = ops.Streams.get("aux", dev)
            aux.wait_stream(c.main_stream)
            with torch.cuda.stream(aux):
                self._critics(c)
        else:
            self._critics(c)
        self._fwd_masks(c)
        self._fwd_reconstruction(c)
        self._bwd_reconstruction(c)
        self._priors(c)
        self._bwd_mask_decoder(c)
        # the critics' block (aux stream) must be complete from here on: g_adv, the critic losses and their gradients (JOIN_TIMING: timed)
        self.sync.join("join", names=("aux",))
        self.sync.segment_done([k for k in ("mi0_discriminator", "mi1_discriminator", "mi_estimator") + N.EXTRA_48C if k in c.keys])
        self._bwd_pose(c)
        # ---- gradient all-reduce (data parallel) + TF Adam per key
        self.sync.segment_done([k for k in ("encoder_0",) if k in c.keys])
        self.sync.finish(c.keys)
        new = self._next_state(c)
        if self._ema is not None:       # every key's Adam is enqueued and joined on this stream; behind the state update, so that
            self._ema_step(graph_lr)    # under data parallelism it is part of the LAST graph of the captured sequence.  No collective.
        build_logs = self._log_thunk(c)
        st = c.st
        if graph_lr is not None:        # graph mode: state lives in fixed device scalars, python counters advance outside
            losses_now, log = build_logs()
            # the logged state is the PRE-update value in both modes: snapshot before the in-place update below
            for k, v in list(log.items()):
                if torch.is_tensor(v) and any(v is sv for sv in st.values()):
                    log[k] = v.clone()
            self._set_logs(losses_now, log)
            for k in st:
                if new[k] is not st[k]:
                    st[k].copy_(new[k])
        else:
            self._lazy_logs = build_logs        # (the closure holds the PRE-update state dict `st`: self.state is replaced, not modified)
            self.state = new
            self.global_step += 1
        self._debug = {"l_mean": c.lm, "l": c.l, "m": c.m, "hard": c.hard, "px": c.px, "generated": c.gen.detach(),
                       "feat": c.feat.detach(), "dl_tot": c.dl_tot, "dl_rec": c.dl_rec, "g_hard0": c.g_hard0, "g_hard1": c.g_hard1,
                       "pe": c.pe2}
        if self.graph is not None and self.graph.capturing:     # the capture owns these buffers: every replay refills them, _graph_step renders from them
            self.graph.img_src = self._image_sources(c)
        elif self._want_images:
            self._render_images(self._image_sources(c), c.step)
        return _LazyLosses(self)

    def _adam(self, keys, graph_lr):
        """One fused TF-Adam launch per key on the current stream (Appendix A.12); advances the keys' step counters (eager mode)."""
        bank = self.model.bank
        lr = self.learning_rate()
        lr_scale = self.probe.get("lr_scale") or {}
        if graph_lr is not None and lr_scale:
            raise NotImplementedError("probe.lr_scale is an eager-mode option (hip_graph: False)")
        # the kernel route: ups_grad_guard directly before the key's Adam ON THE STREAM THIS RUNS ON (EARLY_ADAM: the
        # weight-gradient stream), ups_adam_guarded reading the record.  Taken in graph mode and under `skip_nonfinite`, when there is
        # something to guard; the eager torch route below stays as it was with both off.
        guarded = self._guarded(graph_lr)
        for k in keys:
            grp = bank.groups[k]
            f = grp["flat"]
            rec = None
            if guarded:     # (data parallel: the bucket has been all-reduced, every rank decides alike; 1/world as in Adam)
                rec = self._guard_rec[self._guard_index[k]]
                ops.grad_guard(f["g"], rec, 1.0 / self.world_size, self.grad_clip_norm, self.skip_nonfinite)
                self._guard_used = True
            if graph_lr is not None:
                lr_t = graph_lr
            else:
                t = grp["t"] + 1
                lr_t = lr * lr_scale.get(k, 1.0) * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)
                if self.grad_clip_norm > 0 and not guarded:     # tf.clip_by_global_norm over the key's variables (device side, no sync)
                    gn = torch.linalg.vector_norm(f["g"]) / self.world_size
                    f["g"].mul_(torch.clamp(self.grad_clip_norm / gn.clamp_min(1e-30), max=1.0))
            ops.adam_step(f["p"], f["g"], f["m"], f["v"], lr_t, self.beta1, self.beta2, self.adam_eps, 1.0 / self.world_size, guard=rec)
            # enqueued: this key's weights and counter have moved (for _after_failed_step, key by key).  AFTER the call: adam_step raises on
            # a rejected argument or a refused launch, i.e. with nothing enqueued; an asynchronous fault cannot be pinned to a key anyway
            if graph_lr is None:
                grp["t"] = t
                self.sync.stepped.add(k)

    def _guarded(self, graph_lr):
        """Does a step with this `graph_lr` run the guard kernels?  Under `skip_nonfinite` always; for `grad_clip_norm` alone only in
        graph mode (eager clipping without `skip_nonfinite` stays on the torch route, bit for bit as before).  With both keys unset:
        never -- the step's launches are then exactly the earlier ones."""
        return self.skip_nonfinite or (graph_lr is not None and self.grad_clip_norm > 0)

    def guard_report(self):
        """The guard records as python numbers (synchronises): {optimizer key: {skipped, clipped, consecutive (cumulative, this
        process, since construction), nonfinite, norm, scale (the most recent step)}, "state": {skipped, consecutive}}.  All zero
        (scale 0.0) for a key whose guard has not run."""
        torch.cuda.synchronize(self.device)
        rec, out = self._guard_rec.cpu(), OrderedDict()
        for k, i in self._guard_index.items():
            r = ops.guard_read(rec[i])
            out[k] = {n: r[n] for n in ("skipped", "clipped", "consecutive", "nonfinite", "norm", "scale")}
        s = self._guard_state.cpu().tolist()
        out["state"] = {"skipped": int(s[0]), "consecutive": int(s[1])}
        return out

    # ------------------------------------------------------------------ weight EMA
    def _ema_init(self):
        """One shadow bucket per optimizer key (keys under `fix_weights` have none), a copy of the weights; per-variable views of the
        shadows under the variables' names; the update counts and the kernel's scratch; the item arrays without and with guard records."""
        bank, d = self.model.bank, self.device
        keys = self.loss_keys()
        shadow = OrderedDict((k, bank.groups[k]["flat"]["p"].detach().clone()) for k in keys)
        views = OrderedDict()
        for k in keys:
            off = 0
            for n in bank.groups[k]["names"]:
                cnt = bank.params[n].numel()
                views[n] = shadow[k][off:off + cnt].view(bank.params[n].shape)
                off += cnt
        rec = lambda k, guarded: self._guard_rec[self._guard_index[k]] if guarded else None
        items = {g: ops.EmaItems([(shadow[k], bank.groups[k]["flat"]["p"].detach(), rec(k, g)) for k in keys]) for g in (False, True)}
        self._ema = {"keys": keys, "shadow": shadow, "views": views, "items": items,
                     "n": torch.zeros(len(keys), dtype=torch.int64, device=d), "omd": torch.zeros(len(keys), dtype=torch.float32, device=d)}

    def _ema_step(self, graph_lr):
        """The step's one ops.ema_update (two launches for all keys), behind every key's Adam on the launching stream.  Under the guarded
        step the items carry the keys' records: a key that did not step keeps its shadow and its count."""
        e = self._ema
        ops.ema_update(e["items"][bool(self._guarded(graph_lr))], e["n"], e["omd"], self.ema_decay, self.ema_warmup)

    def ema_report(self):
        """{optimizer key: updates its shadow has taken} (synchronises).  ValueError with `ema_decay` off."""
        if self._ema is None:
            raise ValueError("ema_report: the weight EMA is off (ema_decay: 0)")
        torch.cuda.synchronize(self.device)
        return OrderedDict(zip(self._ema["keys"], (int(x) for x in self._ema["n"].cpu().tolist())))

    def ema_state(self):
        """The shadows by variable name, as host copies (the checkpoint's form)."""
        return OrderedDict((n, t.detach().cpu().clone()) for n, t in self._ema["views"].items())

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the scope the model's weights ARE the shadows (every ``TrainModel`` method runs on them); the weights proper wait in
        the shadow buckets and return, bit for bit, on exit: ops.ema_swap + ops.weights_changed each way, no copy of the buckets.  No
        training step inside the scope.  ValueError with `ema_decay` off, and under `precision: fp8`, where refreshing the converted
        copies advances the delayed scales (the refusal `val_freq` makes)."""
        if self._ema is None:
            raise ValueError("ema_weights: the weight EMA is off (ema_decay: 0)")
        if self.model.fp8.enabled:
            raise ValueError("ema_weights cannot be combined with precision: fp8: refreshing the converted weight copies advances the "
                             "delayed scales, so the scope would move the next training step's scales")
        ops.Fp8.activate(self.model.fp8)
        items = self._ema["items"][False]
        ops.ema_swap(items)
        ops.weights_changed(self.model.nets.prep)
        try:
            yield self
        finally:
            ops.ema_swap(items)
            ops.weights_changed(self.model.nets.prep)

    @torch.no_grad()
    def _restore_ema(self, shadows, counts, keep, where):
        """After a restore of the weights.  shadows: {variable name: tensor} from the file, or None; counts: {key: int}, an int for
        every key, or None.  `use_ema`: the weights are overwritten by the file's shadows.  With the feature on the shadows start as the
        restored weights, counts 0, and take the file's shadows and counts over them where it holds some."""
        bank = self.model.bank
        if shadows is not None:
            shadows = {n: (t if torch.is_tensor(t) else torch.from_numpy(t)) for n, t in shadows.items()
                       if n in keep and n in bank.params and tuple(t.shape) == tuple(bank.params[n].shape)}
        if self.use_ema:
            if not shadows:
                raise ValueError("use_ema: True, but {} holds no shadow weights of this model".format(where))
            bank.load(shadows)
        if self._ema is None:
            return
        e = self._ema
        for k in e["keys"]:
            e["shadow"][k].copy_(bank.groups[k]["flat"]["p"])
        e["n"].zero_()
        if not shadows:
            msg = "{} holds no shadow weights: the weight EMA starts from the restored weights, counts 0".format(where)
            if self.logger:
                self.logger.info(msg)
            return
        for n, t in shadows.items():
            if n in e["views"]:
                e["views"][n].copy_(t.to(torch.float32))
        if counts is not None:
            vals = [int(counts if isinstance(counts, int) else counts.get(k, 0)) for k in e["keys"]]
            e["n"].copy_(torch.tensor(vals, dtype=torch.int64))

    def dp_wait_ms(self):       # (bench.py reports it)
        return self.sync.dp_wait_ms()

    # ------------------------------------------------------------------ image logs (model.py:968-1053; SB_model48c:1038-1094)
    def _image_sources(self, c):
        """References to the step's tensors the canvases are rendered from (nothing is launched or allocated here)."""
        raw = getattr(c, "raw_views", None) or (c.v0, c.v1, c.vt)
        src = {"B": c.B, "P": c.P, "df": c.df, "inputs": raw, "views": (c.v0, c.v1, c.vt), "tps": self.model.use_tps,
               "lm": c.lm, "m": c.m, "hard": c.hard, "bits": c.hbits, "gen": c.gen.detach(), "feat": c.feat.detach()}
        if c.df:        # SB_model48c:1057-1059
            src["single"] = OrderedDict((nm, c.crit[k][1].detach()) for nm, k in
                                        (("global_generated", "d_single"), ("alpha_generated", "d_alpha"), ("pi_generated", "d_pi")))
        return src

    def _image_state(self):
        if self._img is None:
            dev = self.device
            side = torch.cuda.Stream(dev)
            with torch.cuda.stream(side):
                colors = torch.from_numpy(IL.mask_color_bytes(IL.mask_colors01(self.model.n_parts))).to(dev)
                table = torch.from_numpy(IL.viridis_bytes()).to(dev)
            self._img = {"stream": side, "colors": colors, "table": table, "writer": None}
        return self._img

    def _release_images(self):
        """The canvases of the previous image step read tensors of that step (and, under hip_graph, buffers the next replay refills)
        on the side stream: the launching stream is ordered behind them -- an event wait on the device, no host synchronisation --
        before those tensors are released.  Nothing to do after a step that rendered no images."""
        if self._img_hold is not None:
            _, done = self._img_hold
            torch.cuda.current_stream(self.device).wait_event(done)
            self._img_hold = None

    @torch.no_grad()
    def _render_images(self, src, step):
        """Fill ``img_ops`` with the reference's image logs of this step as uint8 device canvases [H, W, 3 | 1] -- what edflow's logging
        hook writes as PNG files: 4-D img_ops with more than one image tiled (cols=None), values quantised by
        uint8(clamp((v + 1) * 127.5, 0, 255)) (UNVERIFIED, see csrc/canvas.hip; maps in [0,1] -- level sets, edge sets, masks,
        p_heatmap -- therefore lie between gray and white).  Reporting only: no generator draw, no optimizer or state update, no host
        synchronisation.  `cross` (model.py:488-500) is decoded on the launching stream -- the decoder's workspaces are not shared
        between streams -- with the weights as the step left them; everything else runs on a side stream behind an event."""
        model, dev = self.model, self.device
        st = self._image_state()
        B, P, df = src["B"], src["P"], src["df"]
        main, side = torch.cuda.current_stream(dev), st["stream"]
        hard, bits, m = src["hard"], src["bits"], src["m"]
        cross = None
        if ops.Fp8.enabled:       # a further forward pass would feed the delayed activation scales of the training step
            IL.warn_once(self.logger, "cross-fp8", "log_images: `cross` is not rendered under precision: fp8")
        else:
            pi, ai = reversed_indices(B, P)
            cross = model.decode_mixed(hard[:B], src["feat"], pi, ai, chunk=B)
        side.wait_stream(main)
        out = OrderedDict()
        with torch.cuda.stream(side):
            soft = ops.part_softmax(src["lm"][:B], None, want_hard=False)[1]          # out_parts_soft (model.py:468-469)
            out["out_parts_soft_visualization"] = ops.canvas_mask_rgb(st["colors"], mask=soft)
            out["m0_sample_visualization"] = ops.canvas_mask_rgb(st["colors"], mask=m[:B])
            for name, sl in (("encoding_masks_visualization", slice(B, 2 * B)), ("decoding_masks_visualization", slice(0, B))):
                if bits is not None:
                    out[name] = ops.canvas_mask_rgb(st["colors"], bits=bits[sl], n_parts=P, cols=B)
                else:
                    out[name] = ops.canvas_mask_rgb(st["colors"], mask=hard[sl], one_hot=True, cols=B)
            first = ops.canvas_first_item(m[0], st["table"], hard=hard[0] if bits is None else None, bits=None if bits is None else bits[0])
            out["masks"] = first[3]
            v0, v1, _ = src["views"]
            if bits is not None:
                out["assigned_parts"] = ops.canvas_assigned_parts(v0, v1, bits0=bits[:B], bits1=bits[B:], n_parts=P)
            else:
                out["assigned_parts"] = ops.canvas_assigned_parts(v0, v1, hard0=hard[:B], hard1=hard[B:])
            if df:
                for name, g_img in src["single"].items():
                    out[name] = ops.canvas_images(g_img)
            else:
                out["mumford_sha_edges"], out["p_heatmap"], out[IL.LEVELS_TITLE] = first[1], first[2], first[0]
            for name, v in zip(("view0", "view1") if df else ("view0", "view1", "view0_target"), src["inputs"]):
                out[name] = ops.canvas_images(v)
            if cross is not None:
                out["cross"] = ops.canvas_images(cross)
            out["generated"] = ops.canvas_images(src["gen"])
            if src["tps"] and not df:       # model.py:1046-1053
                for name, v in zip(("tps_view0", "tps_view1", "tps_view0_target"), src["views"]):
                    out[name] = ops.canvas_images(v)
            # the step's own outputs, as TrainModel.outputs names them (views of the step's tensors: valid until the next step)
            model._last = {"generated": src["gen"][..., :3].float(), "m0_sample": m[:B], "out_parts_soft": soft,
                           "encoding_mask": hard[B:], "decoding_mask": hard[:B]}
            if cross is not None:
                model._last["cross"] = cross
            done = side.record_event()
        self.img_ops = out
        self._img_step = step
        self._img_hold = (src, done)

    def fetch_images(self):
        """{name: uint8 array [H,W,3] or [H,W,1]} of the most recent image step (empty before the first)."""
        if self._img is None:
            return OrderedDict()
        self._img["stream"].synchronize()
        return OrderedDict((k, v.cpu().numpy()) for k, v in self.img_ops.items())

    def _write_images(self, step):
        """<root>/train/<name>_<step:07>.png for every canvas (rank 0): device-to-host copies on the side stream into pinned buffers,
        PNG encoding on the writer's thread (imglog.ImageWriter: bounded queue, blocks when full)."""
        if not self.root or self.rank != 0 or not self.img_ops:
            return
        if not IL.have_pil():
            IL.warn_once(self.logger, "no-pil", "log_images: PIL is not installed: no image logs are written")
            return
        st = self._image_state()
        if st["writer"] is None:
            st["writer"] = IL.ImageWriter(self.root)
        with torch.cuda.stream(st["stream"]):
            host = OrderedDict()
            for k, v in self.img_ops.items():
                host[k] = torch.empty(v.shape, dtype=torch.uint8, pin_memory=True)
                host[k].copy_(v, non_blocking=True)
            ready = st["stream"].record_event()
        st["writer"].submit(step, host, ready)

    def _flush_images(self, close=False):
        w = self._img["writer"] if self._img is not None else None
        if w is not None:
            if close:
                w.close()
                self._img["writer"] = None
            else:
                w.flush()

    # ------------------------------------------------------------------ edflow iterate(): log cadence of LoggingHook
    def fetch_logs(self):
        out = OrderedDict()
        for k, v in self.log_ops.items():
            out[k] = float(v) if torch.is_tensor(v) else float(v)
        out.update(self._val_logs)      # the val/ keys of the most recent validation (`val_freq`)
        self._check_tps_singular()      # (the floats above have synchronised already)
        if getattr(self, "_guard_used", False):     # the kernel route of the optimizer step has run: its records (cumulative counts, the last step's norm)
            rep = self.guard_report()
            for k in self._guard_index:
                out["guard/skipped_" + k], out["guard/clipped_" + k] = rep[k]["skipped"], rep[k]["clipped"]
                out["guard/grad_norm_" + k], out["guard/clip_scale_" + k] = rep[k]["norm"], rep[k]["scale"]
            out["guard/state_skipped"] = rep["state"]["skipped"]
        return out

    def tps_singular_count(self):
        """`use_tps`: samples so far whose TPS system was singular and that were left unwarped (synchronises)."""
        return 0 if self._tps_singular is None else int(self._tps_singular.item())

    def _check_tps_singular(self):
        if self._tps_singular is None or self._tps_warned:
            return
        n = self.tps_singular_count()
        if n:
            self._tps_warned = True
            msg = ("use_tps: {} sample(s) had a singular thin-plate-spline system (coincident control points) and kept the identity "
                   "transform (reported once per run)".format(n))
            if self.logger:
                self.logger.warning(msg)
            else:
                warnings.warn(msg)

    # ------------------------------------------------------------------ periodic validation (`val_freq`, `val_csv`)
    def _init_validation(self):
        """On rank 0, the validation set(s) and evaluators of `val_metrics`: decoded once, kept as pinned uint8 (the refusals were checked
        when __init__ began)."""
        cfg = self.config
        check_validation_config(cfg)
        if self.rank != 0:              # rank 0 validates; the others meet it at the next step's first collective
            return
        from . import data as _data
        from . import evalutil
        metrics = validation_metrics(cfg)
        self._val = {"metrics": metrics}
        if "iou" in metrics:
            vs = _data.ValidationSet(cfg)
            ev = evalutil.PartEvaluator(self.model, int(cfg.get("eval_n_labels", 32)), lut=cfg.get("eval_label_lut"))
            self._val.update({"set": vs, "evaluator": ev})
        if "reconstruction" in metrics or "parts" in metrics or "equivariance" in metrics or "coherence" in metrics:
            # the label-free metrics: one forward per chunk of B pairs (reconstruction, parts); equivariance takes the chunk's view0
            self._val["pairs"] = _data.ValidationPairs(cfg)
            if "reconstruction" in metrics:
                self._val["rec"] = evalutil.ReconstructionEvaluator(self.device)
            if "parts" in metrics:
                self._val["usage"] = evalutil.PartUsageEvaluator(self.device, self.model.n_parts,
                                                                 float(cfg.get("val_min_part_area", 0.005)))
            if "coherence" in metrics:
                self._val["coherence"] = evalutil.CoherenceEvaluator(self.device, self.model.n_parts, *coherence_config(cfg))
            if "equivariance" in metrics:
                # one warp per validation image, drawn ONCE from a CPU generator seeded by `val_seed` (row i: image i) -- nothing is
                # drawn from the trainer's generators.  Singular systems count where `use_tps` counts them.
                if self._tps_singular is None:
                    self._tps_singular = torch.zeros(1, dtype=torch.int32, device=self.device)
                TPS.base_points(self.device)
                self._val["equiv"] = evalutil.EquivarianceEvaluator(self.device, self.model.n_parts, equivariance_tps_parameters(cfg),
                                                                    n_singular=self._tps_singular)
                self._val["equiv_uniforms"] = evalutil.equivariance_uniforms(len(self._val["pairs"]),
                                                                             cfg.get("val_seed", 1)).to(self.device)

    @torch.no_grad()
    def validate(self):
        """The metrics of `val_metrics` on the validation set under the CURRENT weights -> {"val/...", "val/steps_done"}, also kept for
        ``fetch_logs``.  iou (the default): part IoU (evalutil.PartEvaluator: ``model.segment`` + ups_part_confusion) -> "val/overall",
        "val/iou_<label>"; reconstruction / parts: ``_validate_pairs``, which needs no label images.  Runs on the main stream
        between two steps, draws nothing from the trainer's generators and touches neither optimizer nor Lagrangian / EMA state: the training
        trajectory is the same with and without it.  One host synchronisation per evaluator (the copy of its counts or sums)."""
        if self._val is None:
            return OrderedDict()
        if getattr(self, "val_use_ema", False):      # `val_use_ema`: the same metrics on the shadow weights (getattr: stub trainers of the host tests)
            with self.ema_weights():
                return self._validate()
        return self._validate()

    def _validate(self):
        logs = OrderedDict()
        if "evaluator" in self._val:
            vs, ev = self._val["set"], self._val["evaluator"]
            ev.reset()
            chunk = 2 * int(self.config["batch_size"])
            for c0 in range(0, len(vs), chunk):
                c1 = min(len(vs), c0 + chunk)
                ev.update(vs.float_views(c0, c1, self.device), vs.labels[c0:c1])
            res = ev.result()
            logs["val/overall"] = res["overall"]
            for g in sorted(res["iou"]):
                logs["val/iou_{}".format(g)] = res["iou"][g]
        if "pairs" in self._val:
            logs.update(self._validate_pairs())
        logs["val/steps_done"] = self.global_step       # which weights the numbers belong to: they stay in fetch_logs until the next report
        self._val_logs = logs
        return logs

    def _validation_perceptual(self):
        """What ``_perceptual_view`` needs of a step's context, fixed for validation: the 224 x 224 window of `resize256_crop224` has its
        corner at (16, 16), the centre, instead of a draw from the trainer's generator."""
        c = _Step()
        c.pmode = self.perceptual_input
        if c.pmode not in PERCEPTUAL_INPUTS:
            raise NotImplementedError("perceptual_input: {} ({})".format(c.pmode, " | ".join(PERCEPTUAL_INPUTS)))
        S = int(self.config["spatial_size"])
        if c.pmode != "native" and S not in (128, 256):
            raise NotImplementedError("perceptual_input: {} is restated for 128x128 and 256x256 inputs only (got {})".format(c.pmode, S))
        c.resize2x = c.pmode != "native" and S == 128
        c.crop_yx = None
        if c.pmode == "resize256_crop224":
            c.crop_yx = torch.tensor([16, 16], dtype=torch.int32, device=self.device)
        return c

    def _validate_pairs(self):
        """The label-free metrics of `val_metrics` over the pair set: ONE ``model.forward(chunk, noise=None)`` per chunk of batch_size
        pairs feeds both evaluators.  reconstruction: `generated` against view0 -> val/mse, val/l1, val/psnr, val/ssim
        (ups_image_metrics) and val/rec, the step's own reconstruction term (``_perceptual_view`` + ``vgg.loss`` with `gram_weight`) on
        those tensors, averaged over the chunks.  parts: out_parts_soft / out_parts_hard -> val/part_area_<p>, val/parts_active,
        val/confidence, val/entropy (ups_part_usage).  equivariance: the chunk's view0 against its warped copy, one more pass of the pose
        path per chunk and no forward of its own (``evalutil.EquivarianceEvaluator``) -> val/equiv_agreement, val/equiv_miou,
        val/equiv_iou_<p>, val/equiv_tv, val/equiv_valid.  coherence: the connected components of out_parts_hard (``evalutil.CoherenceEvaluator``;
        listed without reconstruction / parts it runs ``model.segment`` itself) -> val/fragmentation, val/fragmentation_<p>,
        val/components_<p>, val/specks.  One copy to the host per evaluator, and one for val/rec."""
        from . import evalutil
        val, model = self._val, self.model
        pairs, rec, usage, equiv, coher = val["pairs"], val.get("rec"), val.get("usage"), val.get("equiv"), val.get("coherence")
        for ev in (rec, usage, equiv, coher):
            if ev is not None:
                ev.reset()
        B = pairs.batch_size
        pc = self._validation_perceptual() if rec is not None else None
        rec_terms = []
        for ci in range(pairs.chunks()):
            chunk = pairs.chunk_views(ci, self.device)
            if equiv is not None:
                equiv.update(model, chunk["view0"], val["equiv_uniforms"][ci * B:(ci + 1) * B])
            if rec is None and usage is None:
                if coher is not None:               # listed without reconstruction / parts: a pass of the pose path of its own
                    coher.update(model.segment(chunk["view0"]))
                continue
            out = model.forward(chunk, noise=None)
            if rec is not None:
                gen = model.generated_act
                rec.update(gen, chunk["view0"])
                tgt = chunk["view0"] if pc.pmode == "native" else self._perceptual_view(pc, model.to_act(chunk["view0"]))
                rec_terms.append(self.vgg.loss(tgt.contiguous(), self._perceptual_view(pc, gen), model.act_dtype,
                                               gram_weight=self.gram_weight).detach().double().reshape(1))
            if usage is not None:
                usage.update(out["out_parts_soft"], out["out_parts_hard"])
            if coher is not None:
                coher.update(out["out_parts_hard"])
        rec_loss = float(torch.cat(rec_terms).mean()) if rec_terms else None
        return evalutil.validation_logs(rec.result() if rec is not None else None, usage.result() if usage is not None else None, rec_loss,
                                        equiv=equiv.result() if equiv is not None else None,
                                        coherence=coher.result() if coher is not None else None)

    def iterate(self, batch_iterator, num_steps=None, log_fn=print):
        """edflow's session loop with its hooks.  LoggingHook cadence as cub/train/log.txt:221-860 shows it (an IntervalHook whose
        interval doubles after every trigger up to ``log_freq``): global steps 0, 2, 4, 8, ..., 128, then every ``log_freq``
        (250, 500, ...); the keys are printed in alphabetical order with ``global_step`` among them (log.txt:204-263), followed
        by the ``project root`` line."""
        cfg = self.config
        num_steps = num_steps if num_steps is not None else cfg.get("num_steps", 1000000)
        log_freq, ckpt_freq = cfg.get("log_freq", 250), cfg.get("ckpt_freq", 10000)
        interval = 1
        log_fn("[INFO] [Trainer]: " + self.switches_report)
        for batch in batch_iterator:
            if self.global_step >= num_steps:
                break
            s = self.global_step
            log_now = s % interval == 0
            if log_now and self.log_images:     # images on exactly the steps that log scalars
                self.train_step(batch, images=True)
                self._write_images(s)
            else:
                self.train_step(batch)
            # `val_freq`: after the K-th, 2K-th, ... step (global_step counts the steps done); on a step that logs, its lines carry the
            # fresh numbers, on any other step the val/ keys get lines of their own
            val_freq = getattr(self, "val_freq", 0)
            val_now = val_freq > 0 and self.global_step % val_freq == 0 and self._val is not None
            if val_now:
                val = self.validate()
                if not log_now:
                    for k in sorted(val):
                        log_fn("[INFO] [LoggingHook]: {}: {}".format(k, val[k]))
            if log_now:
                interval = min(2 * interval, max(1, log_freq))
                logs = self.fetch_logs()
                logs["global_step"] = s
                for k in sorted(logs):
                    log_fn("[INFO] [LoggingHook]: {}: {}".format(k, logs[k]))
                if self.root:
                    log_fn("[INFO] [LoggingHook]: project root: {}".format(os.path.join(self.root, "train")))
                # failure detection on log steps only (the step itself never synchronises with the host).  Losses are per rank:
                # the decision is made collective, so that every rank of a data-parallel run leaves together instead of the
                # healthy ones waiting in the next all-reduce until the RCCL timeout
                bad = [k for k, v in logs.items() if k.startswith("loss_") and not math.isfinite(v)]
                if getattr(self, "skip_nonfinite", False):      # (getattr: stub trainers of the host tests, as val_freq above)
                    self._check_skipped(bad, s, log_fn)
                else:
                    flag = torch.tensor([1.0 if bad else 0.0], dtype=torch.float32, device=self.device)
                    D.sum_flag(flag, self.world_size, self.process_group)
                    if float(flag) > 0:
                        raise FloatingPointError("non-finite {} at global step {} (on {} rank(s))".format(
                            ", ".join(bad) if bad else "loss on another rank", s, int(float(flag))))
            # edflow CheckpointHook: the file is named after the global step the restored run continues FROM
            if ckpt_freq and self.global_step % ckpt_freq == 0:
                self._flush_images()      # a checkpoint is reported only once the images of the steps before it are on disk
                self._checkpoint()
        self._flush_images(close=True)
        self._checkpoint()                # final state at loop exit

    def _check_skipped(self, bad, s, log_fn):
        """`skip_nonfinite` on a step that logs: the device has kept the bad gradients out of the weights, so non-finite losses `bad` are
        reported once per run instead of ending it; FloatingPointError once some optimizer key (or the state update) has been skipped
        `nonfinite_max_consecutive` times in a row -- decided collectively, as the plain check is."""
        if bad and not self._nonfinite_warned:
            self._nonfinite_warned = True
            msg = ("non-finite {} at global step {}: skip_nonfinite leaves the affected optimizer keys unstepped (reported once per "
                   "run; guard/skipped_<key> counts them)".format(", ".join(bad), s))
            if self.logger:
                self.logger.warning(msg)
            else:
                log_fn("[WARNING] [Trainer]: " + msg)
        rep = self.guard_report()
        stuck = sorted(k for k, r in rep.items() if r["consecutive"] >= self.nonfinite_max_consecutive)
        flag = torch.tensor([1.0 if stuck else 0.0], dtype=torch.float32, device=self.device)
        D.sum_flag(flag, self.world_size, self.process_group)
        if float(flag) > 0:
            raise FloatingPointError("skip_nonfinite: {} skipped {} or more steps in a row by global step {} (on {} rank(s))".format(
                ", ".join(stuck) if stuck else "an optimizer key on another rank", self.nonfinite_max_consecutive, s, int(float(flag))))

    def _checkpoint(self):
        """model.ckpt-<step> of THIS process's current state: written to a temporary name and renamed, so a file of that name
        left by an earlier (or diverged) run in the same project root is replaced, never kept."""
        if not self.root or self.rank != 0:
            return
        path = os.path.join(self.root, "train", "checkpoints", "model.ckpt-{}".format(self.global_step))
        if self._last_ckpt == (path, self.global_step):
            return                        # this very state was just written (loop exit right after a periodic checkpoint)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = path + ".tmp-{}".format(os.getpid())
        self.save_checkpoint(tmp)
        os.replace(tmp, path)
        self._last_ckpt = (path, self.global_step)
