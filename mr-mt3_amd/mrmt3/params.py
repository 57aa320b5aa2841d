"""Flat parameter store for the MR-MT3 models.

All weights of a model live in ONE contiguous fp32 buffer (master copy) laid out in state-dict
order, with matching flat buffers for gradients, AdamW moments and the bf16 shadow the MFMA kernels
read.  Consequences that matter on MI355X:
  * q|k|v, cross k|v and wi_0|wi_1 are adjacent, so the fused [1152,512] / [768,512] / [2048,512]
    GEMM operands are plain views — no concatenation, no copies;
  * AdamW is one kernel launch over the whole model (45.9 M / 48.5 M elements);
  * the data-parallel gradient exchange all-reduces contiguous slices of one buffer over RCCL.
`nn.Parameter`s handed to PyTorch (state_dict, optimizers, Lightning) are views into the master
buffer, so the reference's state-dict schema is preserved byte for byte.
"""
from __future__ import annotations

import fnmatch
from collections import OrderedDict

import torch

from . import lib
from .synthetic import state_dict_shapes


# state-dict aliases of the model classes (module.py): a pattern that matches the alias names the tensor itself
ALIASES = {"encoder.embed_tokens.weight": "proj.weight", "decoder.embed_tokens.weight": "decoder_embed_tokens.weight",
           "segmem_encoder.embed_tokens.weight": "segmem_proj.weight"}


def match_keys(keys, patterns, what: str) -> set:
    """Canonical keys of `keys` that one of the fnmatch `patterns` matches (an alias of ALIASES counts for its tensor).
    A pattern that matches nothing is a ValueError naming it."""
    if patterns is None:
        return set()
    if isinstance(patterns, str):
        raise ValueError("%s must be a list of patterns, got the string %r" % (what, patterns))
    keys = list(keys)
    names = [(k, k) for k in keys] + [(a, k) for a, k in ALIASES.items() if k in set(keys)]
    out = set()
    for pat in patterns:
        if not isinstance(pat, str):
            raise ValueError("%s: a pattern is a string, got %r" % (what, pat))
        hit = {k for name, k in names if fnmatch.fnmatchcase(name, pat)}
        if not hit:
            raise ValueError("%s: the pattern %r matches no parameter" % (what, pat))
        out |= hit
    return out


def ema_decay_option(ema_decay):
    """None (off) or a float in (0, 1); anything else is a ValueError."""
    if ema_decay is None:
        return None
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 < float(ema_decay) < 1.0:
        raise ValueError("ema_decay must be None or a number in (0, 1), got %r" % (ema_decay,))
    return float(ema_decay)


class ParamGroups:
    """Which tensors train and with which hyper-parameters: `frozen` / `no_decay` lists of fnmatch patterns over the
    state-dict keys, `lr_scale` {pattern: factor} (a later pattern overrides an earlier one).  Host only."""

    def __init__(self, keys, frozen=None, no_decay=None, lr_scale=None):
        keys = list(keys)
        self.patterns = dict(frozen=list(frozen or []), no_decay=list(no_decay or []),
                             lr_scale=dict(lr_scale or {}))
        self.frozen = match_keys(keys, frozen, "frozen")
        self.no_decay = match_keys(keys, no_decay, "no_decay")
        self.scale = {}
        if lr_scale is not None and not isinstance(lr_scale, dict):
            raise ValueError("lr_scale must map a pattern to a factor, got %r" % (lr_scale,))
        for pat, f in (lr_scale or {}).items():
            if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 <= float(f) < float("inf"):
                raise ValueError("lr_scale[%r] must be a finite number >= 0, got %r" % (pat, f))
            for k in match_keys(keys, [pat], "lr_scale"):
                self.scale[k] = float(f)
        if len(self.frozen) == len(keys):
            raise ValueError("frozen: every parameter is frozen, nothing is left to train")

    @property
    def trivial(self) -> bool:
        """No option given: the one-group step of before."""
        return not (self.frozen or self.no_decay or self.scale)

    def hyper(self, key, weight_decay):
        """(weight_decay, lr_scale) of a trainable tensor."""
        return (0.0 if key in self.no_decay else float(weight_decay)), self.scale.get(key, 1.0)

    def ranges(self, flat, weight_decay):
        """[(begin, end, weight_decay, lr_scale)] over the flat buffer in its own order: one entry per run of adjacent
        trainable tensors with equal hyper-parameters."""
        out = []
        for key, off in flat.offsets.items():
            if key in self.frozen:
                continue
            n = flat.numel_of(key)
            wd, sc = self.hyper(key, weight_decay)
            if out and out[-1][1] == off and out[-1][2] == wd and out[-1][3] == sc:
                out[-1] = (out[-1][0], off + n, wd, sc)
            else:
                out.append((off, off + n, wd, sc))
        return out


class FlatParams:
    def __init__(self, cfg: dict, segmem_num_layers: int = 0, device="cpu"):
        self.cfg = cfg
        self.shapes = state_dict_shapes(cfg, segmem_num_layers)
        self.offsets: "OrderedDict[str, int]" = OrderedDict()
        off = 0
        # Flat order = state-dict order, except that the cross-attention k|v projections of ALL decoder layers sit
        # together in front of decoder block 0: they all multiply the same encoder output, so the forward projects it for
        # every layer in one [n_layers * 768, 512] GEMM and the backward returns its gradient in one GEMM with
        # K = n_layers * 768 ("decoder.ckv_all"); the per-layer [768, 512] views stay valid.
        n_dec = cfg["num_decoder_layers"]
        ckv = [f"decoder.block.{i}.layer.1.EncDecAttention.{n}.weight" for i in range(n_dec) for n in ("k", "v")]
        ckv_set = set(ckv)
        order = []
        for k in self.shapes:
            if k in ckv_set:
                continue
            if k == "decoder.block.0.layer.0.SelfAttention.q.weight":
                order.extend(ckv)
            order.append(k)
        assert len(order) == len(self.shapes)
        for k in order:
            self.offsets[k] = off
            n = 1
            for s in self.shapes[k]:
                n *= s
            off += n
        self.numel = off
        assert off % 4 == 0
        self.P = torch.zeros(off, dtype=torch.float32, device=device)   # master
        self.G = None          # gradients (lazily allocated)
        self.M = None          # AdamW exp_avg
        self.V = None          # AdamW exp_avg_sq
        self.S = None          # bf16 shadow of P
        self.ST = None         # pre-transposed bf16 weights for dgrad
        self.E = None          # EMA of P (f32), when the trainer keeps one
        self.opt_ranges = None  # lib.OptRanges of the trainable tensors (None: one group, everything trains)
        self.frozen = frozenset()   # canonical keys without a gradient (Engine.wgrad and friends skip them)
        self._shadow_version = -1
        # tensors other than P whose in-place updates also change the master (the nn.Parameter views of
        # MT3Module: after `.to(device)` each owns a version counter of its own, so torch.optim / load_state_dict
        # writes do not bump P._version)
        self.version_sources = ()
        self._frozen_spans = None
        self._build_groups(segmem_num_layers)

    # ---- fused weight groups ------------------------------------------------------------------------
    def _build_groups(self, segmem_num_layers):
        cfg = self.cfg
        d, inner, dff = cfg["d_model"], cfg["d_kv"] * cfg["num_heads"], cfg["d_ff"]
        g: "OrderedDict[str, tuple]" = OrderedDict()   # name -> (offset, rows, cols)

        def add(name, first_key, rows, cols):
            g[name] = (self.offsets[first_key], rows, cols)

        def stack(prefix, n, dec):
            for i in range(n):
                b = f"{prefix}.block.{i}.layer"
                add(f"{prefix}.{i}.qkv", f"{b}.0.SelfAttention.q.weight", 3 * inner, d)
                add(f"{prefix}.{i}.o", f"{b}.0.SelfAttention.o.weight", d, inner)
                ff = 1
                if dec:
                    add(f"{prefix}.{i}.cq", f"{b}.1.EncDecAttention.q.weight", inner, d)
                    add(f"{prefix}.{i}.ckv", f"{b}.1.EncDecAttention.k.weight", 2 * inner, d)
                    add(f"{prefix}.{i}.co", f"{b}.1.EncDecAttention.o.weight", d, inner)
                    ff = 2
                add(f"{prefix}.{i}.wi", f"{b}.{ff}.DenseReluDense.wi_0.weight", 2 * dff, d)
                add(f"{prefix}.{i}.wo", f"{b}.{ff}.DenseReluDense.wo.weight", d, dff)

        add("proj", "proj.weight", d, d)
        stack("encoder", cfg["num_layers"], False)
        stack("decoder", cfg["num_decoder_layers"], True)
        if cfg["num_decoder_layers"] > 0:
            add("decoder.ckv_all", "decoder.block.0.layer.1.EncDecAttention.k.weight", cfg["num_decoder_layers"] * 2 * inner, d)
        add("lm_head", "lm_head.weight", cfg["vocab_size"], d)
        if segmem_num_layers:
            add("segmem_proj", "segmem_proj.weight", d, d)
            stack("segmem_encoder", segmem_num_layers, False)
        self.groups = g
        # pre-transposed (dgrad) copies: every group but proj (the mel input needs no gradient) and the per-layer
        # cross k|v views (their dgrad is the one K = n_layers * 768 product against "decoder.ckv_all")
        self.t_offsets = OrderedDict()
        off = 0
        for name, (_, r, c) in g.items():
            if name == "proj" or (name.startswith("decoder.") and name.endswith(".ckv")):
                continue
            self.t_offsets[name] = off
            off += r * c
        self.t_numel = off

    # ---- views ---------------------------------------------------------------------------------------
    def view(self, buf, key):
        shp = self.shapes[key]
        n = 1
        for s in shp:
            n *= s
        o = self.offsets[key]
        return buf[o:o + n].view(shp)

    def numel_of(self, key):
        n = 1
        for s in self.shapes[key]:
            n *= s
        return n

    def master(self, key):
        return self.view(self.P, key)

    # ---- parameter groups ----------------------------------------------------------------------------
    def set_groups(self, groups, weight_decay):
        """Install (or, with None / a trivial spec, remove) the range table of `groups` (a ParamGroups)."""
        if groups is None or groups.trivial:
            self.opt_ranges, self.frozen = None, frozenset()
            return None
        tab = lib.OptRanges(groups.ranges(self, weight_decay), self.numel)
        if self.P.is_cuda:
            tab.to(self.P.device)
        self.opt_ranges, self.frozen = tab, frozenset(groups.frozen)
        return tab

    def all_range(self, weight_decay):
        """The table of the one-group step (EMA without any other option)."""
        tab = lib.OptRanges([(0, self.numel, float(weight_decay), 1.0)], self.numel)
        if self.P.is_cuda:
            tab.to(self.P.device)
        self.opt_ranges, self.frozen = tab, frozenset()
        return tab

    def is_frozen(self, t) -> bool:
        """Does the gradient tensor `t` (a contiguous view of G) lie wholly inside frozen tensors?  (A fused q|k|v view
        with only some members frozen does not: its gradient is computed, the frozen part is never read.)"""
        if not self.frozen or self.G is None:
            return False
        if self._frozen_spans is None or self._frozen_spans[0] is not self.frozen:
            spans = []
            for a, b in sorted((self.offsets[k], self.offsets[k] + self.numel_of(k)) for k in self.frozen):
                if spans and spans[-1][1] == a:
                    spans[-1][1] = b
                else:
                    spans.append([a, b])
            self._frozen_spans = (self.frozen, spans, [a for a, _ in spans])
        import bisect
        off = (t.data_ptr() - self.G.data_ptr()) // 4
        _, spans, starts = self._frozen_spans
        i = bisect.bisect_right(starts, off) - 1
        return i >= 0 and spans[i][0] <= off and off + t.numel() <= spans[i][1]

    def trainable_spans(self):
        """Merged [begin, end) element spans of the tensors that train (whatever their hyper-parameters)."""
        out = []
        for key, off in self.offsets.items():
            if key in self.frozen:
                continue
            n = self.numel_of(key)
            if out and out[-1][1] == off:
                out[-1] = (out[-1][0], off + n)
            else:
                out.append((off, off + n))
        return out

    def all_frozen(self, prefix: str) -> bool:
        """Is every tensor whose key starts with `prefix` frozen?"""
        if not self.frozen:
            return False
        ks = [k for k in self.shapes if k.startswith(prefix)]
        return bool(ks) and all(k in self.frozen for k in ks)

    def ensure_ema(self):
        """The EMA buffer, a copy of P when first switched on."""
        if self.E is None or self.E.device != self.P.device:
            self.E = self.P.detach().clone()
        return self.E

    def grad(self, key):
        return self.view(self.G, key)

    def W(self, name, dtype):
        """Fused weight [rows, cols] in the compute dtype."""
        o, r, c = self.groups[name]
        buf = self.S if dtype == torch.bfloat16 else self.P
        return buf[o:o + r * c].view(r, c)

    def WT(self, name):
        """Pre-transposed bf16 weight [cols, rows] (dgrad operand)."""
        _, r, c = self.groups[name]
        o = self.t_offsets[name]
        return self.ST[o:o + r * c].view(c, r)

    def GW(self, name):
        o, r, c = self.groups[name]
        return self.G[o:o + r * c].view(r, c)

    # ---- device / shadows --------------------------------------------------------------------------
    def to(self, fn):
        self.P = fn(self.P)
        for n in ("G", "M", "V", "E"):
            b = getattr(self, n)
            if b is not None:
                setattr(self, n, fn(b))
        self.S = None
        self.ST = None
        self._shadow_version = -1
        if self.opt_ranges is not None and self.P.is_cuda:
            self.opt_ranges.to(self.P.device)
        if self.P.dtype != torch.float32:
            raise TypeError("MR-MT3 master weights stay fp32; pick the compute dtype on the model")

    def ensure_grads(self):
        if self.G is None or self.G.device != self.P.device:
            self.G = torch.zeros_like(self.P)
        return self.G

    def ensure_adam(self):
        if self.M is None or self.M.device != self.P.device:
            self.M = torch.zeros_like(self.P)
            self.V = torch.zeros_like(self.P)

    def master_version(self):
        """Changes whenever the master weights were written through P or through any registered view."""
        v = self.P._version
        for t in self.version_sources:
            v += t._version
        return v

    def refresh_shadows(self, force=False, need_transposed=True):
        """(Re)build the bf16 shadow and the transposed dgrad copies when the master changed."""
        if not self.P.is_cuda:
            raise RuntimeError("bf16 shadows live on the GPU (no CPU fallback)")
        ver = self.master_version()
        have_t = self.ST is not None
        if not force and self.S is not None and ver == self._shadow_version and (have_t or not need_transposed):
            return
        if self.S is None or self.S.device != self.P.device:
            self.S = torch.empty(self.numel, dtype=torch.bfloat16, device=self.P.device)
        if force or ver != self._shadow_version or self._shadow_version < 0:
            lib.cast(self.P, self.S)
        if need_transposed:
            self.refresh_transposed()
        self._shadow_version = ver

    def refresh_transposed(self):
        """Rebuild every pre-transposed dgrad weight from the bf16 shadow in ONE launch."""
        import numpy as np
        if self.ST is None or self.ST.device != self.P.device:
            self.ST = torch.empty(self.t_numel, dtype=torch.bfloat16, device=self.P.device)
            self._tr_tab = None
        if getattr(self, "_tr_tab", None) is None:
            rec, starts, tot = [], [], 0
            for name, (o, r, c) in self.groups.items():
                if name not in self.t_offsets:
                    continue
                rec.append((o, self.t_offsets[name], r, c))
                starts.append(tot)
                tot += ((r + 63) // 64) * ((c + 63) // 64)       # 64x64 tiles (csrc/layout.hip TRB)
            tab = np.zeros(len(rec), dtype=[("src", "<i8"), ("dst", "<i8"), ("rows", "<i4"), ("cols", "<i4")])
            for i, t in enumerate(rec):
                tab[i] = t
            self._tr_tab = torch.from_numpy(tab.view(np.uint8).copy()).to(self.P.device)
            self._tr_start = torch.tensor(starts, dtype=torch.int32, device=self.P.device)
            self._tr_n, self._tr_tiles = len(rec), tot
        lib.transpose_batched(self.S, self.ST, self._tr_tab, self._tr_start, self._tr_n, self._tr_tiles)

    def adamw_step(self, lr_dev, step_dev, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=1.0, stat_dev=None,
                   clip_value=0.0, ema_decay=None):
        """torch.optim.AdamW semantics over the whole model in one launch; keeps shadows current.  With a range table
        installed (set_groups / all_range) only its elements step, weight decay and lr factor come from the table
        (`weight_decay` is not passed on) and, with `ema_decay`, the EMA of P follows in the same launch.  `stat_dev`: under
        the clip coefficient / skip flag that lib.grad_norm left there, with an optional clamp of the scaled gradient to
        +-clip_value; a skipped step rewrites the transposed shadows from the unchanged bf16 shadow: the same bits."""
        tab = self.opt_ranges
        if ema_decay is not None and tab is None:
            raise RuntimeError("adamw_step: ema_decay needs a range table (FlatParams.all_range / set_groups)")
        self.ensure_adam()
        if self.S is None:
            self.refresh_shadows()
        lib.adamw_step(self.P, self.G, self.M, self.V, lr_dev, step_dev, betas[0], betas[1], eps,
                       weight_decay if tab is None else None, grad_scale, shadow=self.S, stat=stat_dev, clip_value=clip_value,
                       ranges=None if tab is None else tab.to(self.P.device),
                       ema=None if ema_decay is None else self.ensure_ema(), ema_decay=ema_decay or 0.0)
        self.refresh_transposed()
        self._shadow_version = self.master_version()

    def load_numpy(self, weights: dict):
        for k, v in weights.items():
            self.master(k).copy_(torch.from_numpy(v).to(self.P.device))
