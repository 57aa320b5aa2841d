"""CPU reference of the optimizer parameter groups: torch.optim.AdamW with REAL param groups on f32 copies of the
weights (frozen tensors are simply not handed to it, as `requires_grad=False` parameters would not be), and the EMA
recurrence as a plain loop in float64.  Used by tests/test_optim_groups_cpu.py and tests/test_optim_groups_gpu.py."""
import fnmatch

import numpy as np
import torch

ALIASES = {"encoder.embed_tokens.weight": "proj.weight", "decoder.embed_tokens.weight": "decoder_embed_tokens.weight",
           "segmem_encoder.embed_tokens.weight": "segmem_proj.weight"}


def match(keys, patterns):
    """Canonical keys matched by any of the fnmatch patterns (an alias names its tensor)."""
    keys = list(keys)
    names = [(k, k) for k in keys] + [(a, k) for a, k in ALIASES.items() if k in keys]
    return {k for pat in (patterns or []) for name, k in names if fnmatch.fnmatchcase(name, pat)}


def small_cfg(**over):
    """The smallest model the engine accepts that still has more than one layer per stack."""
    from mrmt3.synthetic import T5_SMALL
    return dict(T5_SMALL, num_layers=2, num_decoder_layers=2, **over)


class TorchGroups:
    """torch.optim.AdamW over f32 CPU copies of `weights` {key: tensor}, param groups [decay, no_decay] (each only when
    non-empty), keys of a group in `order`; `frozen` keys are in no group.  step(grads) takes {key: tensor} gradients."""

    def __init__(self, weights, order, frozen=(), no_decay=(), lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8):
        self.p = {k: torch.nn.Parameter(weights[k].detach().float().cpu().clone()) for k in order}
        self.frozen, self.no_decay = set(frozen), set(no_decay)
        self.order = list(order)
        self.opt = self._make(lr, weight_decay, betas, eps)
        self.hyper = (lr, weight_decay, betas, eps)

    def _make(self, lr, weight_decay, betas, eps):
        dec = [self.p[k] for k in self.order if k not in self.frozen and k not in self.no_decay]
        nod = [self.p[k] for k in self.order if k not in self.frozen and k in self.no_decay]
        groups = [dict(params=dec, weight_decay=weight_decay)] if dec else []
        if nod:
            groups.append(dict(params=nod, weight_decay=0.0))
        return torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps)

    def set_frozen(self, frozen):
        """A new frozen set between steps: a new optimizer over the new groups that keeps every tensor's state (moments
        and step count), which is what un-freezing a parameter and re-adding it with its old state amounts to."""
        old = {id(p): s for p, s in self.opt.state.items()}
        self.kept = getattr(self, "kept", {})
        self.kept.update(old)
        self.frozen = set(frozen)
        self.opt = self._make(*self.hyper)
        for p in self.p.values():
            if id(p) in self.kept and any(p is q for g in self.opt.param_groups for q in g["params"]):
                self.opt.state[p] = self.kept[id(p)]

    def step(self, grads, lr=None):
        for k, p in self.p.items():
            p.grad = None if k in self.frozen else grads[k].detach().float().cpu().clone()
        if lr is not None:
            for g in self.opt.param_groups:
                g["lr"] = lr
        self.opt.step()

    def weights(self):
        return {k: p.detach() for k, p in self.p.items()}


def ema64(trajectory, decay, start):
    """ema_t = ema_{t-1} + (1 - decay) * (p_t - ema_{t-1}) in float64 over a list of float arrays; `1 - decay` is the f32
    difference the kernel forms (exact for an f32 decay >= 0.5, Sterbenz), so only the recurrence's own roundings differ."""
    om = float(np.float32(1.0) - np.float32(decay))
    e = np.asarray(start, dtype=np.float64).copy()
    for p in trajectory:
        e = e + om * (np.asarray(p, dtype=np.float64) - e)
    return e
