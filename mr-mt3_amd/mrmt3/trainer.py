"""Training step of the MI355X path: audio -> log-mel -> forward -> fused CE -> hand-written backward
(overlapped with the RCCL gradient exchange) -> one-launch AdamW.

This is the build's counterpart of what `train.py:43-103` gets from `pl.Trainer.fit` +
`MT3Net*.training_step` + `configure_optimizers` (tasks/mt3_net.py:27-68): same loss, same
optimizer semantics (torch.optim.AdamW defaults, cosine-warmup LambdaLR stepped per batch), one
process per GPU.  Nothing on the host waits for the device inside a step: the learning rate, the
step counter and the loss stay in device memory.

Host out of the step.  After two eager steps of a given input shape the whole step — ≈700 kernel launches on one
stream — is captured into hipGraphs and replayed: the host then enqueues a handful of
graph launches per step instead of ≈600 ctypes calls (19.6 of 28 ms per step in round 1).  What makes the replay equal
to the eager step bit for bit:
  * dropout masks are keyed by (seed, site, DEVICE step counter): the site ids restart at 0 every step and the
    kernels read `step_dev`, which AdamW increments, so frozen by-value arguments still give new masks each step;
  * the learning rate is written to `lr_dev` (device) before the replay, outside the graph;
  * inputs are copied into static buffers the captured kernels read.
With more than one rank the step is cut into one graph per gradient bucket: the RCCL all-reduce of a finished bucket
is enqueued EAGERLY between two replays on the launch stream, so it still overlaps the rest of backward and no
collective is ever captured.  That is the default, because it is the form that needs nothing from RCCL but a plain call.

Captured collectives (one graph with the all-reduces in-line; two graphs side by side with flag hand-offs) were built and
measured in round 5 and lost (+0.13-0.25 ms exposed / +3.2-3.8 ms: profiles/r05_collectives_ab.txt); round 6 took them out of
the product (profiles/tools/closed/trainer_captured_collectives_r5.py keeps the code for the record).

A capture that fails.  Whatever trips a capture (a kernel that refuses, an illegal call inside it), the step goes on with plain
launches — and nothing of the failed capture may stay behind, because of how torch 2.10 / ROCm 7.2 behave (round 6 root cause of
the round-5 abort, profiles/r06_capture_abort_root_cause.txt): (1) the cyclic garbage collector running INSIDE a capture frees
older trainers' graphs, page-locked tables and communicators — HIP calls that are illegal while the thread captures — and
invalidates the capture; (2) `CUDAGraph.capture_begin` on a stream that is still in capture mode raises AFTER the graph has noted
the default generator's state but BEFORE that state has noted the graph, and destroying such a graph object throws inside
`~CUDAGraph` -> std::terminate -> SIGABRT.  So: garbage is collected BEFORE a capture and the collector is off during it; a
capture never begins on a stream whose status is not "none" (mrmt3_stream_capture_status); after a failure every participating
stream is taken out of capture mode (mrmt3_stream_abandon_capture), the capture stream is replaced by a fresh one, and a graph
object whose capture_begin raised is never destroyed (`_retire`).

Packed decoder rows (`pack_targets=True`, MRMT3_PACK_TARGETS=1; mrmt3/packing.py).  The step reads each row's length on the
host (from CPU labels directly, else one device-to-host copy of B int32 — the one place a packed step waits for the device),
picks the capacity Tcap, and runs the decoder, the lm_head and the CE on Tcap packed rows; Tcap = B*L takes the dense step
unchanged.  The signature of a captured step gains Tcap; the pack kernel runs inside the graph on the static label buffer.
Captured packed signatures are kept in a small LRU (MRMT3_PACK_GRAPHS, default 4).  Eviction follows the rules above: the
device is drained and the graph dropped OUTSIDE any capture, and the garbage is collected before the next capture begins.

Gradient accumulation (`accumulate_grad_batches=N`, Lightning's automatic-optimisation semantics).  `train_step` consumes one
micro-batch; the optimizer steps after every N-th, or at `finish_accumulation()` for a partial cycle (an epoch's end).  With
N > 1 a step has three phases, each its own part of the captured signature: "first" zeroes G and runs forward + backward,
"middle" runs forward + backward, "last" runs forward + backward with the bucket cuts and exchanges, then AdamW.  N = 1 is
the single phase of before (signature, graphs and launches unchanged).  The gradient producers all add into `flat.G`, so
after the last micro-batch G holds the SUM over micro-batches (and, after the exchange, over ranks) of the per-micro-batch
mean gradients; AdamW takes grad_scale = 1/(world*N), which is Lightning's loss/N per micro-batch — also for a partial cycle.
Dropout salt: `step_dev` counts optimizer steps (AdamW's bias correction); with N > 1 the dropout kernels read `salt_dev`
instead, a device counter of micro-batches bumped at the end of every micro-batch inside the step (mrmt3_counter_add), so
the micro-batches of one cycle and every replay draw their own masks, the same in eager and replayed steps.  With N = 1
`salt_dev` IS `step_dev`: the masks are those of the plain step.

Gradient clipping, gradient norm, non-finite guard (`gradient_clip_val`, `gradient_clip_algorithm`, `skip_nonfinite`,
`track_grad_norm`; Lightning's Trainer arguments of the first two names).  When any of the four is set, the optimizer tail
of a step — plain step, "last" phase, finish_accumulation() — is mrmt3_grad_norm + mrmt3_adamw_step with `stat_dev` instead
of the plain mrmt3_adamw_step: the norm of G * 1/(world*N) (the mean gradient over ranks and micro-batches, after the exchange) is
reduced on the device in a fixed order, the clip coefficient and the skip flag stay in device memory (`_clip_stat`) and
AdamW reads them there, so the captured tail graph clips by this step's norm on every replay and the host never waits.
Every rank holds the same G after the all-reduce and reduces it in the same order: same coefficient, no extra collective.
A skipped step (non-finite norm under skip_nonfinite) leaves P, M, V and the shadows untouched; `step_dev` still advances —
it counts ATTEMPTED optimizer steps and stays equal to host_step, so the dropout salt moves on and checkpoints need no new
field (AdamW's bias correction counts the skipped step: negligible after warm-up).  With all four off nothing changes:
the same calls, graphs and launches as before.

Label smoothing and z-loss (`label_smoothing`, `z_loss`).  With either non-zero the CE of the training step is
mrmt3_ce_fwd_bwd_reg / mrmt3_lmhead_ce_fwd_bwd_reg: the objective (1-eps)*nll + eps*(lse - mean logit) + z*lse^2 per scored
row, its gradient, and the plain NLL beside it.  Both are by-value launch arguments fixed at construction: they are part of
the captured step and of no signature.  `train_step` returns the objective (`last_loss`), `last_nll` is the plain NLL; both
are handled alike (device scalars, one per micro-batch, reduced over ranks).  `eval_loss` stays the plain NLL.  With both
zero the old entry points run — the same launches as before — and `last_nll` is `last_loss`.

Parameter groups and EMA weights (`frozen`, `no_decay`, `lr_scale`, `ema_decay`).  The patterns are fnmatch patterns
over the state-dict keys.  With any of them given the optimizer tail is mrmt3_adamw_step (and mrmt3_grad_norm when the
clipping tail is on) over a device table of the trainable ranges: a frozen tensor is never read or written, gets no
weight gradient (Engine.wgrad drops it, so the grouped launch plans fewer items), no place in a gradient bucket, and when the
whole encoder is frozen the backward stops at the cross-attention k|v projections.  The table is device memory read by
pointer: the captured step follows it.  `set_frozen()` changes the set between steps and drops the captured graphs (two
eager warm-up steps, then a new capture); moments are never zeroed, a re-thawed tensor resumes with the ones it had.  With
`ema_decay` the same launch keeps `flat.E`, the EMA of the weights (`ema_state_dict()`, `with trainer.ema_weights():`).  With
none of the four given nothing changes: the same calls, graphs and launches as before.
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.distributed as dist

from . import lib
from .ddp import GradBuckets
from .params import ALIASES, ParamGroups, ema_decay_option


_RETIRED = []


def _retire(graph) -> None:
    """A CUDAGraph whose capture_begin raised must never be destroyed: torch 2.10's ~CUDAGraph un-registers the graph from the
    generator state it noted in capture_begin, and when capture_begin raised between the two registrations that check throws
    inside the destructor and the process aborts.  One reference is leaked on purpose (a few hundred bytes)."""
    import ctypes
    _RETIRED.append(graph)
    ctypes.pythonapi.Py_IncRef(ctypes.py_object(graph))


def _first_line(e) -> str:
    t = str(e)
    return t.splitlines()[0] if t else ""


CLIP_ALGORITHMS = ("norm", "value")


def clip_options(gradient_clip_val=None, gradient_clip_algorithm="norm", skip_nonfinite=False, track_grad_norm=False):
    """Validate the clipping arguments (host only) -> (on, max_norm, clip_value, skip): `on` iff any of the four asks for
    the norm / clip / guard tail; max_norm > 0 clips by global norm, clip_value > 0 clamps by value, 0 = off."""
    if gradient_clip_algorithm is None:
        gradient_clip_algorithm = "norm"
    if gradient_clip_algorithm not in CLIP_ALGORITHMS:
        raise ValueError("gradient_clip_algorithm must be one of %s, got %r" % (CLIP_ALGORITHMS, gradient_clip_algorithm))
    if gradient_clip_val is not None:
        if isinstance(gradient_clip_val, bool) or not isinstance(gradient_clip_val, (int, float)):
            raise ValueError("gradient_clip_val must be None or a number > 0, got %r" % (gradient_clip_val,))
        if not gradient_clip_val > 0 or gradient_clip_val == float("inf"):
            raise ValueError("gradient_clip_val must be None or a finite number > 0, got %r" % (gradient_clip_val,))
    val = 0.0 if gradient_clip_val is None else float(gradient_clip_val)
    by_value = gradient_clip_algorithm == "value"
    on = gradient_clip_val is not None or bool(skip_nonfinite) or bool(track_grad_norm)
    return on, (0.0 if by_value else val), (val if by_value else 0.0), bool(skip_nonfinite)


class _CapturedStep:
    """One input signature's captured step: graph segments (each followed by the gradient buckets to send), the tail
    graph (AdamW) and the static tensors the graphs read and write."""

    def __init__(self):
        self.segments, self.tail = [], None
        self.inputs = self.labels = self.prev = self.loss = self.nll = None


class Trainer:
    def __init__(self, model, lr: float = 2e-4, lr_lambda=None, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, weighted_loss: bool = False, layers_per_bucket: int = 4,
                 graph: bool = None, grad_exchange_dtype=None, pack_targets: bool = None,
                 accumulate_grad_batches: int = 1, gradient_clip_val=None, gradient_clip_algorithm: str = "norm",
                 skip_nonfinite: bool = False, track_grad_norm: bool = False, label_smoothing: float = 0.0,
                 z_loss: float = 0.0, frozen=None, no_decay=None, lr_scale=None, ema_decay=None):
        self.ema_decay = ema_decay_option(ema_decay)
        self._ema_swapped = False
        self.loss_reg, self.label_smoothing, self.z_loss = lib.ce_options(label_smoothing, z_loss)
        self.clip_on, self._max_norm, self._clip_value, self.skip_nonfinite = clip_options(
            gradient_clip_val, gradient_clip_algorithm, skip_nonfinite, track_grad_norm)
        n_acc = int(accumulate_grad_batches)
        if n_acc < 1 or n_acc != accumulate_grad_batches:
            raise ValueError("accumulate_grad_batches must be an integer >= 1, got %r" % (accumulate_grad_batches,))
        self.accumulate = n_acc
        self._micro = 0                  # micro-batches of the current accumulation cycle already run
        if pack_targets is None:
            pack_targets = os.environ.get("MRMT3_PACK_TARGETS", "0") != "0"
        self.pack_targets = bool(pack_targets)
        if self.pack_targets and model.engine.variant == "segmem_v1":
            raise ValueError("pack_targets is not supported for segmem_v1: its memory slots are prepended to the decoder input, "
                             "so the decoder rows cannot be cut to the scored prefix")
        self.model, self.flat, self.engine = model, model.flat, model.engine
        self.groups = ParamGroups(model.flat.shapes, frozen, no_decay, lr_scale)      # (host only: raises before anything is built)
        assert model.device.type == "cuda", "the trainer drives the HIP kernels: move the model to the GPU first"
        self.base_lr, self.lr_lambda = lr, lr_lambda
        self.betas, self.eps, self.wd = betas, eps, weight_decay
        self.weighted = weighted_loss
        dev = model.device
        self.lr_dev = torch.full((1,), lr, device=dev, dtype=torch.float32)
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        self.host_step = 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        cfg = model.cfg
        if grad_exchange_dtype is None and os.environ.get("MRMT3_GRAD_EXCHANGE", "f32") == "bf16":
            grad_exchange_dtype = torch.bfloat16
        # 4 layers per bucket, the last bucket cut down to the encoder's lowest layer + the embedding tables (ddp.py): 5 buckets of
        # 47 / 57 / 38 / 28 / 14 MB for MT3Net (6 with segment memory).  A bucket boundary costs 0.07 ms
        # of step time (a graph segment of its own + the grouped weight-gradient launch split there: 16 / 8 / 4 / 2 buckets =
        # 25.26 / 24.70 / 24.40 / 24.23 ms at one rank with forced collectives, plain step 24.17,
        # profiles/r04_bucket_boundary_cost.txt); the LAST bucket's all-reduce is the one nothing overlaps, so fewer, larger
        # buckets stop paying once that tail outgrows the boundaries saved (2 buckets: the whole encoder, 80 MB, at the end).
        layers_per_bucket = max(1, int(os.environ.get("MRMT3_DDP_LAYERS_PER_BUCKET", layers_per_bucket)))
        self.buckets = GradBuckets(self.flat, cfg["num_layers"], cfg["num_decoder_layers"],
                                   model.segmem_num_layers > 0, layers_per_bucket, exchange_dtype=grad_exchange_dtype)
        self.buckets.before_fire = model.engine.join_wgrad      # the bucket's deferred weight and norm-weight gradients run here
        self.flat.ensure_grads()
        self.flat.ensure_adam()
        if self.world > 1:   # C2: identical replicas
            dist.broadcast(self.flat.P, src=0)
        self._install_groups()
        if self.ema_decay is not None:
            self.flat.E = None
            self.flat.ensure_ema()                           # a copy of P (after the broadcast: the same on every rank)
        self.last_loss = None
        self.last_nll = None             # the plain NLL of the last (micro-)batch; `last_loss` itself when no loss option is on
        # norm / clip coefficient / skip flag of the last optimizer step, the skip counter and the norm kernel's partials:
        # device memory the captured tail reads and writes, allocated here, never inside a capture
        self._clip_stat = self._skipped_dev = self._clip_ws = None
        if self.clip_on:
            self._clip_stat = torch.zeros(4, device=dev, dtype=torch.float32)
            self._skipped_dev = torch.zeros(1, device=dev, dtype=torch.int32)
            self._clip_ws = lib.grad_norm_workspace(dev)
        # every dropout mask of a step is salted in-kernel by a device counter (see module docstring): the optimizer step
        # counter itself, or with accumulation a micro-batch counter of its own
        self.salt_dev = self.step_dev if n_acc == 1 else torch.zeros(1, device=dev, dtype=torch.int32)
        self.engine.step_dev = self.salt_dev
        self.use_graph = (os.environ.get("MRMT3_TRAIN_GRAPH", "1") != "0") if graph is None else bool(graph)
        self._collective_stream_checked = False
        self.graph_warmup = 2            # eager steps per input signature before capture (tables, workspaces)
        self._graphs = {}                # signature -> _CapturedStep
        self._eager_seen = {}
        self._cap_stream = None
        self._cap_owner = None
        self.pack_graphs = max(1, int(os.environ.get("MRMT3_PACK_GRAPHS", "4")))
        self._pack_lru = []              # captured packed signatures, least recently used first

    def mel_from_audio(self, audio):
        """[B, n_samples] f32 device audio -> [B, frames, 512] mel in the compute dtype."""
        from contrib import spectrograms as sp
        return sp.logmel_segments(audio, out_bf16=(self.engine.dt == torch.bfloat16))

    # ---- one step's device work (identical in eager mode, under capture and — by replay — afterwards) ------------
    def _pack_plan(self, labels, tcap):
        """The device packing plan of `labels` at capacity `tcap` (None: the dense step)."""
        if tcap is None:
            return None
        cfg = self.model.cfg
        return lib.pack_plan(labels.contiguous(), tcap, cfg["decoder_start_token_id"], cfg["pad_token_id"])

    def pack_capacity(self, labels):
        """Tcap of this batch, or None for the dense step (packing off, or nothing to save).  Device labels cost one
        device-to-host copy of B int32 (a wait for the device)."""
        if not self.pack_targets:
            return None
        from . import packing
        B, L = labels.shape
        if labels.is_cuda:
            lengths = lib.pack_lengths(labels.contiguous()).cpu().numpy()
        else:
            lengths = packing.row_lengths(labels.numpy())
        tcap = packing.capacity(lengths, B, L)
        return None if tcap == B * L else tcap

    def _phase(self):
        """Phase of the next micro-batch: None without accumulation (the whole optimizer step), else "first" / "middle" /
        "last" of its cycle."""
        if self.accumulate == 1:
            return None
        if self._micro == 0:
            return "first"
        return "last" if self._micro == self.accumulate - 1 else "middle"

    def _step_body(self, inputs, labels, targets_prev, audio, cut=None, tcap=None, phase=None):
        """Enqueues one optimizer step, or with accumulation one micro-batch of it (`phase`, see _phase).  `cut(bucket_indices)`
        is called where a gradient bucket is complete (only when collectives will run, only in a step that ends with AdamW):
        under capture it closes the current graph segment.  tcap: packed decoder rows.  Returns (objective, plain NLL): one
        tensor twice when no loss option is on."""
        eng, flat = self.engine, self.flat
        eng.begin_step()                                     # nothing deferred leaks in; dropout site ids are per-step
        mel = self.mel_from_audio(inputs) if audio else inputs
        plan = self._pack_plan(labels, tcap)
        targets = labels.reshape(-1) if plan is None else plan.targets
        if eng.dt == torch.bfloat16:
            dec, tape = eng.forward(mel, labels, targets_prev, training=True, need_grad=True, want_logits=False, pack=plan)
            # lm_head + CE over row chunks: the f32 logits exist one chunk at a time in a cache-sized workspace
            loss, dl, nll = lib.lmhead_cross_entropy(dec, eng.W("lm_head"), targets, want_grad=True,
                                                     grad_dtype=torch.bfloat16, weighted=self.weighted,
                                                     label_smoothing=self.label_smoothing, z_loss=self.z_loss,
                                                     return_nll=True)
        else:                                                # fp32 engine (`precision: 32`): exact-f32 lm_head, then CE
            logits, tape = eng.forward(mel, labels, targets_prev, training=True, need_grad=True, pack=plan)
            loss, dl, nll = lib.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets, want_grad=True,
                                              grad_dtype=torch.float32, weighted=self.weighted,
                                              label_smoothing=self.label_smoothing, z_loss=self.z_loss, return_nll=True)
        if phase in (None, "first"):
            flat.G.zero_()
        self.buckets.reset()
        if phase in ("first", "middle"):                   # no exchange: the gradients keep accumulating in G
            eng.backward(tape, dl)
        elif cut is None:
            eng.backward(tape, dl, on_layer_done=self.buckets.on_layer_done)
            self.buckets.finish()
        else:
            sent = set()

            def layer_done(prefix, i):
                idx = [j for j in self.buckets.triggered_by(prefix, i) if j not in sent]
                if idx:
                    sent.update(idx)
                    eng.join_wgrad()                         # the segment ends with its bucket's gradients complete
                    cut(idx)
            active = self.buckets.active
            eng.backward(tape, dl, on_layer_done=layer_done if active else None)     # ends with join_wgrad()
            cut([j for j in range(len(self.buckets.buckets)) if j not in sent] if active else [])
        if phase in (None, "last"):
            self._optimizer_tail()
        if self.accumulate > 1:
            lib.counter_add(self.salt_dev, 1)               # the next micro-batch draws other masks
        return loss, nll

    # ---- parameter groups / EMA -----------------------------------------------------------------------------------------
    @property
    def groups_on(self) -> bool:
        """Does the optimizer tail run over a range table (any group option, or EMA)?"""
        return self.flat.opt_ranges is not None

    def _install_groups(self):
        """The range table of `self.groups` in device memory (EMA alone: one range over everything), the trainable slices
        of the gradient buckets; with no option at all: nothing, the one-group step."""
        if self.groups.trivial:
            self.flat.set_groups(None, self.wd)
            if self.ema_decay is not None:
                self.flat.all_range(self.wd)
            self.buckets.set_trainable(None)
        else:
            self.flat.set_groups(self.groups, self.wd)
            self.buckets.set_trainable(self.flat.trainable_spans() if self.groups.frozen else None)

    def _drop_graphs(self):
        """Forget every captured step, outside any capture (see close()); the next steps warm up eagerly and recapture."""
        import gc
        torch.cuda.synchronize()
        self._graphs.clear()
        self._eager_seen.clear()
        self._pack_lru.clear()
        gc.collect()
        torch.cuda.synchronize()

    def set_frozen(self, patterns):
        """Change the frozen set between optimizer steps (None / []: thaw everything).  Nothing is zeroed — a thawed
        tensor continues with the moments it had; the captured graphs are dropped, so the next steps of each input shape
        run eagerly (`graph_warmup`) and are then captured again with the new pruning."""
        if self._micro:
            raise RuntimeError("set_frozen: %d micro-batch(es) of an accumulation cycle are pending" % self._micro)
        if self._ema_swapped:
            raise RuntimeError("set_frozen inside `with trainer.ema_weights()`")
        groups = ParamGroups(self.flat.shapes, patterns, self.groups.patterns["no_decay"], self.groups.patterns["lr_scale"])
        self._drop_graphs()
        self.engine.reset_deferred()
        self.groups = groups
        self._install_groups()

    def ema_state_dict(self):
        """The EMA weights in the model's (= the reference's) state-dict schema, on the CPU."""
        if self.ema_decay is None:
            raise RuntimeError("ema_state_dict: the trainer was built without ema_decay")
        torch.cuda.current_stream().synchronize()
        out = type(self.model.state_dict())()
        for k, v in self.model.state_dict().items():
            key = ALIASES.get(k, k)
            src = self.flat.view(self.flat.E, key) if key in self.flat.shapes else v
            out[k] = src.detach().cpu().clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate / decode / score with the EMA weights: inside the block the master buffer holds the EMA (the buffers
        keep their addresses — parameters, decoder handles and captured graphs all point into them — their contents are
        exchanged), the bf16 shadow and the transposed copies are rebuilt from it; on exit the training weights and their
        shadow come back bit for bit.  Training inside the block is a RuntimeError."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights: the trainer was built without ema_decay")
        if self._ema_swapped:
            raise RuntimeError("ema_weights: already inside the context")
        flat = self.flat
        with torch.no_grad():
            keep_p = flat.P.clone()
            keep_s = None if flat.S is None else flat.S.clone()
            flat.P.copy_(flat.E)
            if flat.S is not None:
                flat.refresh_shadows(force=True, need_transposed=flat.ST is not None)
        self._ema_swapped = True
        try:
            yield self
        finally:
            with torch.no_grad():
                flat.P.copy_(keep_p)
                if keep_s is not None:
                    flat.S.copy_(keep_s)
                    if flat.ST is not None:
                        flat.refresh_transposed()
                    flat._shadow_version = flat.master_version()
                else:
                    flat._shadow_version = -1                # a shadow first made inside the block holds the EMA: recast
            self._ema_swapped = False

    def _no_training_in_ema(self, what):
        if self._ema_swapped:
            raise RuntimeError("%s inside `with trainer.ema_weights()`: the master buffer holds the EMA weights" % what)

    def _optimizer_tail(self):
        """AdamW on the exchanged G (over the range table when one is installed); with clipping / norm tracking / the
        non-finite guard on, the device-side norm first."""
        scale = 1.0 / (self.world * self.accumulate)
        if self.clip_on:
            lib.grad_norm(self.flat.G, scale, self._max_norm, self.skip_nonfinite, self._clip_ws, self._clip_stat,
                          self._skipped_dev, ranges=self.flat.opt_ranges)
        self.flat.adamw_step(self.lr_dev, self.step_dev, self.betas, self.eps, self.wd, grad_scale=scale,
                             stat_dev=self._clip_stat if self.clip_on else None,
                             clip_value=self._clip_value if self.clip_on else 0.0, ema_decay=self.ema_decay)

    @property
    def last_grad_norm(self):
        """Device [1] f32 view (un-synchronised, like last_loss): the global L2 norm of the last optimizer step's mean
        gradient, before clipping.  None when clipping, norm tracking and the non-finite guard are all off."""
        return None if self._clip_stat is None else self._clip_stat[0:1]

    @property
    def skipped_steps(self) -> int:
        """Optimizer steps the non-finite guard skipped (reads the device counter: waits for the device)."""
        return 0 if self._skipped_dev is None else int(self._skipped_dev.item())

    def train_step(self, inputs, labels, targets_prev=None, audio: bool = False):
        """One optimizer step, or with accumulate_grad_batches = N > 1 one micro-batch (the optimizer steps after every N-th).
        `inputs` is mel [B,Le,512] or, with audio=True, raw audio [B,n].  Returns the (device, un-synchronised) mean loss of
        this rank over this (micro-)batch, undivided by N: the objective whose gradient was taken.  With label_smoothing /
        z_loss on, `last_nll` holds the plain NLL of the same (micro-)batch."""
        m, eng = self.model, self.engine
        self._no_training_in_ema("train_step")
        m.train()
        if self.buckets.active and not self._collective_stream_checked:
            # once, before the first exchange: the collectives only overlap the rest of backward if their stream sits on
            # another hardware queue than the compute stream's (profiles/r05_two_graph_probe.txt)
            self._collective_stream_checked = True
            if inputs.is_cuda and not self._pick_collective_stream(torch.cuda.current_stream(), inputs.device):
                import warnings
                warnings.warn("no stream was found that runs side by side with the compute stream: the gradient all-reduces "
                              "will queue behind the backward kernels instead of overlapping them")
        if self.lr_lambda is not None:
            self.lr_dev.fill_(self.base_lr * self.lr_lambda(self.host_step))
        if targets_prev is not None and eng.variant == "segmem_v2_with_prev":
            # in place on the caller's tensor, like the reference (t5_segmem_v2_with_prev.py:119)
            targets_prev.masked_fill_(targets_prev == -100, m.cfg["pad_token_id"])
        tcap = self.pack_capacity(labels)
        if self.pack_targets and not labels.is_cuda:
            labels = labels.to(self.flat.G.device)          # CPU labels: lengths taken above, copied once
        phase = self._phase()
        if self.use_graph:
            loss, nll = self._graph_step(inputs, labels, targets_prev, audio, tcap, phase)
        else:
            loss, nll = self._step_body(inputs, labels, targets_prev, audio, tcap=tcap, phase=phase)
        self._micro += 1
        if self._micro == self.accumulate:
            self._micro = 0
            self.host_step += 1
        if self.world > 1:   # C4: logged loss, reduced without blocking the host
            loss = loss.clone()
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, async_op=True).wait()   # stream-level wait only
            loss /= self.world
            if self.loss_reg:
                nll = nll.clone()
                dist.all_reduce(nll, op=dist.ReduceOp.SUM, async_op=True).wait()
                nll /= self.world
        self.last_loss = loss
        self.last_nll = nll if self.loss_reg else loss
        return loss

    def finish_accumulation(self) -> bool:
        """Run the optimizer step of a partial accumulation cycle (the micro-batches left at an epoch's end, like Lightning):
        exchange the accumulated gradients (not overlapped: backward is over), then AdamW with the same grad_scale
        1/(world*N) as a full cycle.  Nothing happens when no micro-batch is pending.  Returns whether a step ran."""
        if self._micro == 0:
            return False
        self._no_training_in_ema("finish_accumulation")
        if self.lr_lambda is not None:
            self.lr_dev.fill_(self.base_lr * self.lr_lambda(self.host_step))
        self.buckets.reset()
        self.buckets.finish()
        self._optimizer_tail()
        self._micro = 0
        self.host_step += 1
        return True

    @property
    def pending_micro_batches(self) -> int:
        """Micro-batches run since the last optimizer step (0 <= n < accumulate_grad_batches)."""
        return self._micro

    @property
    def optimizer_steps(self) -> int:
        """Optimizer steps taken (what the LR schedule, max_steps and checkpoints count); same as host_step."""
        return self.host_step

    # ---- hipGraph capture / replay of the step ---------------------------------------------------------------
    def _graph_step(self, inputs, labels, targets_prev, audio, tcap=None, phase=None):
        sig = (bool(audio), tuple(inputs.shape), inputs.dtype, tuple(labels.shape),
               None if targets_prev is None else tuple(targets_prev.shape))
        if tcap is not None:
            sig = sig + (tcap,)
        if phase is not None:
            sig = sig + (phase,)
        cap = self._graphs.get(sig)
        if cap is None:
            seen = self._eager_seen.get(sig, 0)
            if seen < self.graph_warmup:
                self._eager_seen[sig] = seen + 1
                return self._step_body(inputs, labels, targets_prev, audio, tcap=tcap, phase=phase)
            if tcap is not None:
                self._evict_packed(self.pack_graphs - 1)
            try:
                cap = self._capture(sig, inputs, labels, targets_prev, audio, tcap, phase)
            except Exception as e:     # noqa: BLE001 — whatever a capture trips over, the eager step is still correct
                # (nothing executed during the failed capture: the step below is the first to run; the launches the
                # aborted capture had deferred are dropped — _after_failed_capture and _step_body reset them)
                import warnings
                state = self._after_failed_capture(e)
                warnings.warn("hipGraph capture of the training step failed (%s: %s)%s; continuing with eager launches"
                              % (type(e).__name__, _first_line(e), state))
                self.use_graph = False
                return self._step_body(inputs, labels, targets_prev, audio, tcap=tcap, phase=phase)
            if tcap is not None:
                self._pack_lru.append(sig)
        elif tcap is not None:
            self._pack_lru.remove(sig)
            self._pack_lru.append(sig)
        self.engine.prepare(True)          # weights written through torch since the last step? rebuild the shadows
        cap.inputs.copy_(inputs, non_blocking=True)
        cap.labels.copy_(labels, non_blocking=True)
        if cap.prev is not None:
            cap.prev.copy_(targets_prev, non_blocking=True)
        self.buckets.reset()
        for graph, fire in cap.segments:
            graph.replay()
            for idx in fire:
                self.buckets.fire(idx)
        self.buckets.wait()
        cap.tail.replay()
        loss = cap.loss.clone()            # the graph's own loss scalars are overwritten by the next replay
        return loss, (cap.nll.clone() if self.loss_reg else loss)

    def _evict_packed(self, keep: int):
        """Drop the least recently used captured packed steps until at most `keep` remain.  Called outside any capture: the
        device is drained first (no replay of the graph may be in flight) and the garbage collected here, while HIP calls are
        legal, not by the collector at some later moment."""
        if len(self._pack_lru) <= keep:
            return
        import gc
        torch.cuda.synchronize()
        while len(self._pack_lru) > keep:
            sig = self._pack_lru.pop(0)
            self._graphs.pop(sig, None)
            self._eager_seen.pop(sig, None)
        gc.collect()
        torch.cuda.synchronize()

    # ---- a capture that failed: leave nothing behind -----------------------------------------------------------------
    def _capture_streams(self):
        """Every stream a capture of the step can have pulled into capture mode (a capture spreads to each stream that waits
        on an event of a capturing one: the capture stream itself, the collective stream and the candidates the stream pick
        made), plus the caller's."""
        out = {"current": torch.cuda.current_stream(), "capture": self._cap_stream, "collective": self.buckets._launch}
        for i, s in enumerate(getattr(self, "_stream_candidates", [])):
            out["candidate%d" % i] = s
        seen, uniq = set(), {}
        for k, v in out.items():
            if v is not None and v.cuda_stream not in seen:
                seen.add(v.cuda_stream)
                uniq[k] = v
        return uniq

    def _drop_capture_stream(self):
        """Forget the capture stream; if it is one of our own, destroy it (an invalidated stream is lost for capturing)."""
        owner, self._cap_owner, self._cap_stream = getattr(self, "_cap_owner", None), None, None
        if owner is not None:
            try:
                torch.cuda.synchronize()
            except RuntimeError:
                pass
            owner.close()

    def _after_failed_capture(self, exc) -> str:
        """Called with the exception of a capture that failed, BEFORE anything else is launched or synchronised.  Ends the
        capture on every stream that is still in capture mode (an exception between capture_begin and capture_end — or a
        capture_end that itself fails on an unjoined stream — leaves streams capturing; a device synchronise is illegal
        then), empties the thread's HIP error slot (the library's launch wrappers report whatever sits there as THEIR launch
        failure: one stale code would fail the retry and every eager launch after it), drops what the engine had deferred,
        then drains the device.  Returns a short state report for the warning; with MRMT3_CAPTURE_LOG=<file> the full report
        (traceback, per-stream capture status, live graph / stream / communicator counts) is appended there."""
        import gc
        import traceback
        left = []
        for name, st in self._capture_streams().items():
            was = lib.stream_abandon_capture(st)
            if was != "none":
                left.append("%s stream was left capturing (%s)" % (name, was))
        pending = lib.runtime_error_pop()
        if pending:
            left.append("pending HIP error %s" % pending)
        self._drop_capture_stream()                          # a later capture (another input shape) gets a fresh stream
        self.engine.begin_step()
        log = os.environ.get("MRMT3_CAPTURE_LOG")
        if log:
            objs = gc.get_objects()
            counts = dict(graphs=sum(isinstance(o, torch.cuda.CUDAGraph) for o in objs),
                          streams=sum(isinstance(o, torch.cuda.Stream) for o in objs),
                          comms=sum(isinstance(o, lib.Comm) for o in objs),
                          trainers=sum(isinstance(o, Trainer) for o in objs))
            with open(log, "a") as f:
                f.write("---- failed capture (world=%d, step=%d)\n%s%s\nlive objects: %s\n"
                        % (self.world, self.host_step,
                           "".join(traceback.format_exception(type(exc), exc, exc.__traceback__)),
                           "; ".join(left) or "no stream left capturing, no pending error", counts))
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:        # a device that cannot be drained: say so in Python instead of going on blind
            raise RuntimeError("the device could not be synchronised after a failed graph capture (%s); state: %s"
                               % (_first_line(e), "; ".join(left) or "clean")) from exc
        return (" [" + "; ".join(left) + "]") if left else ""

    # ---- which stream the collectives run on --------------------------------------------------------------------------
    def _side_by_side(self, compute_stream, collective_stream, timeout_ms: int = 100) -> bool:
        """Do kernels of the two streams run side by side?  A spinning wait on the collective stream, then its signal on
        the compute stream: if the wait times out, both streams feed ONE hardware queue (HIP shares a few queues among
        the streams of a priority).  Eager, 0.1 ms when fine, `timeout_ms` when not."""
        dev = self.flat.G.device
        w = torch.zeros(3, dtype=torch.int32, device=dev)            # flag, seen, err
        torch.cuda.synchronize()
        lib.flag_wait(w[0:1], w[1:2], w[2:3], timeout_ms, stream=collective_stream)
        lib.flag_signal(w[0:1], stream=compute_stream)
        torch.cuda.synchronize()
        return int(w[2].item()) == 0

    def _pick_collective_stream(self, compute_stream, device) -> bool:
        """A collective stream on ANOTHER hardware queue than the compute stream's: on a shared queue an eager all-reduce
        simply queues between the backward kernels and overlaps nothing (profiles/r05_two_graph_probe.txt).  HIP deals the
        streams of one priority over a few queues, so: test the stream the buckets already use, then up to eight fresh ones
        (MRMT3_DDP_STREAM_PRIO: their priority, default normal — a resident kernel on a HIGH-priority queue slows the compute
        graph's launches more, profiles/r05_collectives_ab.txt) and keep the first that passes.  At most nine probes of
        100 ms: under a second in all.  False: none did."""
        prio = int(os.environ.get("MRMT3_DDP_STREAM_PRIO", "0"))
        first = self.buckets.collective_stream(device)
        cands = ([first] if first.priority == prio else []) + [None] * 8
        self._stream_candidates = []
        for c in cands:
            s = c if c is not None else torch.cuda.Stream(device=device, priority=prio)
            self._stream_candidates.append(s)
            if s.cuda_stream != compute_stream.cuda_stream and self._side_by_side(compute_stream, s):
                self.buckets.use_collective_stream(s)
                return True
        return False

    def _capture(self, sig, inputs, labels, targets_prev, audio, tcap=None, phase=None):
        """Record the step once (nothing executes during capture); `train_step` then replays it, this step included."""
        import gc
        eng = self.engine
        cur = torch.cuda.current_stream()
        if self._cap_stream is None:
            # a stream of our own, not one out of torch's pool: a stream that some failed capture left invalidated comes back
            # from that pool (round robin over 32), and ROCm never takes it out of capture mode again
            self._cap_owner = lib.OwnedStream(inputs.device)
            self._cap_stream = self._cap_owner.stream
        cs = self._cap_stream
        st = lib.stream_capture_status(cs)
        if st != "none":                   # (checked again before every segment's capture_begin: see begin())
            raise RuntimeError("the capture stream is still in capture mode (%s): not beginning another capture on it" % st)
        # Garbage first, while HIP calls are legal: an older trainer's graphs (hipGraphExecDestroy), page-locked plan tables
        # (hipHostFree) or communicator freed by the cyclic collector in the MIDDLE of the capture invalidate it ("operation
        # failed due to a previous error during capture" — seen only in long-lived processes with such garbage pending).
        gc.collect()
        torch.cuda.synchronize()           # nothing of the eager steps (collectives included) is in flight during capture
        eng.prepare(True)
        cap = _CapturedStep()
        cap.inputs, cap.labels = inputs.clone(), labels.clone()
        cap.prev = None if targets_prev is None else targets_prev.clone()
        cs.wait_stream(cur)
        pool = None
        state = {"g": None}

        def begin():
            # never on a stream that is not cleanly out of capture mode: torch's capture_begin would raise half-way through
            # its registrations and leave a graph object whose destructor aborts the process (module docstring)
            st = lib.stream_capture_status(cs)
            if st != "none":
                raise RuntimeError("the capture stream is still in capture mode (%s): not beginning another capture on it" % st)
            # thread-local capture mode: the process group's watchdog thread polls the events of earlier collectives
            # (hipEventQuery) whenever it likes; under the default global mode that call is illegal while ANY thread
            # captures and the watchdog takes the process down (seen with RCCL at world size 1, forced collectives)
            g = torch.cuda.CUDAGraph()
            try:
                if pool is None:
                    g.capture_begin(capture_error_mode="thread_local")
                else:
                    g.capture_begin(pool=pool, capture_error_mode="thread_local")
            except Exception:
                _retire(g)
                raise
            state["g"] = g

        def cut(fire):
            nonlocal pool
            g = state["g"]
            state["g"] = None
            g.capture_end()
            if pool is None:
                pool = g.pool()
            cap.segments.append((g, list(fire)))
            begin()

        gc_was = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(cs):
                begin()
                try:
                    cap.loss, cap.nll = self._step_body(cap.inputs, cap.labels, cap.prev, audio, cut=cut, tcap=tcap,
                                                        phase=phase)
                    g, state["g"] = state["g"], None
                    g.capture_end()
                    cap.tail = g
                except Exception:
                    g = state["g"]
                    if g is not None:              # a capture is open: end it here.  If it is already invalidated this raises
                        try:                       # too: _after_failed_capture then takes the stream out of capture mode, and
                            g.capture_end()        # the allocator is told by hand that this capture no longer routes
                        except Exception:          # allocations into its pool (capture_end raised before it got there)
                            try:
                                torch._C._cuda_endAllocateToPool(cap.inputs.device.index or 0, g.pool())
                            except Exception:
                                pass
                    raise
        finally:
            if gc_was:
                gc.enable()
        cur.wait_stream(cs)
        self._graphs[sig] = cap
        return cap

    def close(self):
        """Release what the trainer holds on the device in an order that is safe: drain, drop the captured graphs (their
        executables are destroyed now, not by the garbage collector at some later HIP-illegal moment), then the library's
        communicator if the buckets made one.  The trainer is unusable for graph replay afterwards; eager steps still work."""
        self._drop_graphs()
        self._drop_capture_stream()
        self.buckets.close()

    @property
    def graph_captured(self) -> bool:
        return bool(self._graphs)

    # ---- checkpoint / resume (Lightning `.ckpt` layout, see mrmt3.checkpoint) -------------------------------
    def save_checkpoint(self, path: str, epoch: int = 0):
        """Write weights + AdamW moments + step in the layout the reference's ModelCheckpoint produces, so
        either side can resume from it (`train.py:61-72`).  `.pt` / `.pth` paths get the bare state dict
        (`train.py:105-116`).  Refused while micro-batches of an accumulation cycle are pending: their gradients live
        only in G, which a checkpoint does not hold."""
        from . import checkpoint as ck
        if self._micro:
            raise RuntimeError("save_checkpoint: %d micro-batch(es) of an accumulation cycle are pending (their gradients are "
                               "not part of a checkpoint); call finish_accumulation() first, or save after the cycle's "
                               "optimizer step" % self._micro)
        torch.cuda.current_stream().synchronize()
        if str(path).endswith(".ckpt"):
            torch.save(ck.lightning_checkpoint(self.model, self, epoch), path)
        else:
            torch.save({k: v.detach().cpu() for k, v in self.model.state_dict().items()}, path)

    def resume(self, path: str, strict: bool = False) -> int:
        """Load weights (and, from a `.ckpt`, optimizer moments and the step counter).  Returns the global
        step training continues from."""
        from . import checkpoint as ck
        blob = ck.read_checkpoint(path)
        self._no_training_in_ema("resume")
        self.model.load_state_dict(blob["state_dict"], strict=strict)
        step = 0
        saved = (blob["extra"] or {}).get("groups")
        if saved is not None:            # the run's frozen set and group hyper-parameters (a checkpoint without: as built)
            groups = ParamGroups(self.flat.shapes, saved["frozen"], saved["no_decay"], saved["lr_scale"])
            self._drop_graphs()
            self.groups = groups
            if saved.get("ema_decay") is not None:
                self.ema_decay = ema_decay_option(saved["ema_decay"])
            self._install_groups()
        if self.ema_decay is not None:
            ema = (blob["extra"] or {}).get("ema")
            self.flat.E = None
            self.flat.ensure_ema()       # a checkpoint without an EMA: it restarts from the loaded weights
            if ema is not None:
                for k, v in ema.items():
                    self.flat.view(self.flat.E, k).copy_(v)
        if blob["optimizer"] is not None:
            order = ck.reference_parameter_order(self.model.cfg, self.model.segmem_num_layers)
            step = ck.adamw_state_to_flat(blob["optimizer"], self.flat, order, groups=self.groups, weight_decay=self.wd)
            step = max(step, blob["global_step"])
        self.host_step = step
        self._micro = 0
        self.step_dev.fill_(step)
        if self.accumulate > 1:          # the micro-batch salt; a checkpoint without it: past every salt it can have used
            salt = (blob["extra"] or {}).get("dropout_salt")
            self.salt_dev.fill_(step * self.accumulate if salt is None else int(salt))
        if blob["extra"]:
            self.engine.seed = int(blob["extra"]["dropout_seed"])
            self.engine._stream_ctr = int(blob["extra"]["dropout_stream_ctr"])
        if self.world > 1:
            dist.broadcast(self.flat.P, src=0)
            dist.broadcast(self.flat.M, src=0)
            dist.broadcast(self.flat.V, src=0)
            if self.flat.E is not None:
                dist.broadcast(self.flat.E, src=0)
        return step

    @torch.no_grad()
    def eval_loss(self, inputs, labels, targets_prev=None, audio: bool = False):
        self.model.eval()
        mel = self.mel_from_audio(inputs) if audio else inputs
        tcap = self.pack_capacity(labels)
        if self.pack_targets and not labels.is_cuda:
            labels = labels.to(self.flat.G.device)
        plan = self._pack_plan(labels, tcap)
        targets = labels.reshape(-1) if plan is None else plan.targets
        if self.engine.dt != torch.bfloat16:
            logits, _ = self.engine.forward(mel, labels, targets_prev, training=False, need_grad=False, pack=plan)
            return lib.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets, want_grad=False,
                                     weighted=self.weighted)[0]
        dec, _ = self.engine.forward(mel, labels, targets_prev, training=False, need_grad=False, want_logits=False, pack=plan)
        loss, _ = lib.lmhead_cross_entropy(dec, self.engine.W("lm_head"), targets, want_grad=False,
                                           weighted=self.weighted)
        return loss
