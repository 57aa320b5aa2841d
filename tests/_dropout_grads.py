"""The oracle under the kernels' own dropout masks (tests/test_dropout_grads_cpu.py, tests/test_dropout_grads_gpu.py).

`DropPlan` is the `drop=` argument of oracle/t5_ref.py: it hands out the masks of oracle/dropout_ref.py (the restatement of
the two mask generators, device step salt included) in the order mrmt3/engine.py draws its site ids, so that autograd on
the float64 oracle gives the true gradient of the forward the engine runs with `training=True`.

The site walk (ids start at 1 every step, `Engine.begin_step`; seed 365):
  encoder   "emb" (proj(mel) + sinusoid, flat index over [B*Le, d]), then per layer "att" (softmax probabilities, keyed
            (b, h, q, k)), "o" (the o projection's output before the residual add), "g" (gelu(h0) * h1, flat over
            [rows, d_ff]), "wo"; then "out" (the closing norm's output);
  memory    one layer (the engine's shortcut): no id is drawn.  Any other depth: the generic stack draws its 4 per layer + 1
            ids at p = 0 — identity masks, but the decoder's ids move up; its "emb" draws none either way;
  decoder   "emb" (embedding + sinusoid; segmem_v1: over the concatenated [B*(Ls+Ld), d]), per layer "att", "o", "catt"
            (cross-attention over the Lc keys), "co", "g", "wo"; then "out".
Packed decoder rows (`pack_lengths=`): the row-wise masks of the decoder are keyed by the packed row t (flat index
t * cols + c over the Tcap rows); positions past a row's length take no mask (nothing there reaches a scored position);
the attention masks stay (b, h, q, k) of the row's own positions.
"""
import numpy as np
import torch

from oracle import dropout_ref as dr

SEED = 365                      # Engine.seed


class _Sites:
    """The sites of one stack, see oracle.t5_ref.t5_stack."""

    def __init__(self, plan, prefix, draws, p, packed):
        self.plan, self.prefix, self.draws, self.p, self.packed = plan, prefix, draws, p, packed

    def _sid(self, name):
        if not self.draws or (self.prefix == "segmem_encoder" and name == "emb"):
            return None
        return self.plan._draw(f"{self.prefix}.{name}")

    def rows(self, x, name):
        sid = self._sid(name)
        if sid is None or self.p <= 0.0:
            return x
        plan = self.plan
        if self.packed:                                  # x [B, L, cols] dense, the kernel's rows are the packed ones
            B, L, cols = x.shape
            keep, scale = dr.keep_mask(plan.tcap * cols, self.p, SEED, sid, plan.step)
            keep = keep.reshape(plan.tcap, cols)
            m = np.ones((B, L, cols))
            off = 0
            for b, n in enumerate(plan.pack_lengths):
                m[b, :n] = keep[off:off + n] * float(scale)
                off += n
        else:
            keep, scale = dr.keep_mask(x.numel(), self.p, SEED, sid, plan.step)
            m = keep.reshape(tuple(x.shape)) * float(scale)
        return x * torch.from_numpy(m).to(x.dtype)

    def probs(self, pr, name):
        sid = self._sid(name)
        if sid is None or self.p <= 0.0:
            return pr
        B, H, Lq, Lk = pr.shape
        keep, scale = dr.attn_keep_mask(B, H, Lq, Lk, self.p, SEED, sid, self.plan.step)
        return pr * torch.from_numpy(keep * float(np.float32(scale))).to(pr.dtype)


class DropPlan:
    """p: the dropout rate; step: the value of the device step counter the kernels read (None: no counter attached);
    swap {k: id}: the k-th drawn site (0-based, in walk order) takes stream id `id` instead of its own k + 1;
    pack_lengths / tcap: the decoder runs on packed rows of these lengths at this capacity.  `names` lists the drawn sites."""

    def __init__(self, p, step=None, swap=None, pack_lengths=None, tcap=None):
        self.p, self.step, self.swap = float(p), step, dict(swap or {})
        self.pack_lengths = None if pack_lengths is None else [int(n) for n in pack_lengths]
        self.tcap = tcap
        self.names = []

    def _draw(self, name):
        k = len(self.names)
        self.names.append(name)
        return self.swap.get(k, k + 1)

    def stack(self, prefix, n_layers):
        if prefix == "segmem_encoder":
            return _Sites(self, prefix, draws=n_layers != 1, p=0.0, packed=False)
        return _Sites(self, prefix, draws=True, p=self.p, packed=prefix == "decoder" and self.pack_lengths is not None)


def weights64(cfg, segmem_num_layers=0, grad=True):
    """The golden weights of `cfg` in float64."""
    from mrmt3.synthetic import golden_weights
    return {k: torch.from_numpy(v).double().requires_grad_(grad) for k, v in golden_weights(cfg, segmem_num_layers).items()}


def oracle_loss(sd, cfg, mel, lab, variant="t5", prev=None, segmem_num_layers=1, drop=None):
    """(loss, logits) of the float64 oracle."""
    from oracle import t5_ref
    logits = t5_ref.forward_logits(sd, cfg, mel.double(), lab, variant=variant, targets_prev=None if prev is None else prev.clone(),
                                   segmem_num_layers=segmem_num_layers, drop=drop)
    return t5_ref.ce_loss(logits, lab), logits


def oracle_grads(cfg, mel, lab, variant="t5", prev=None, segmem_num_layers=None, drop=None, sd=None):
    """One forward + backward of the float64 oracle under `drop`: (loss, logits, {name: gradient or None})."""
    if segmem_num_layers is None:
        segmem_num_layers = 0 if variant == "t5" else 1
    if sd is None:
        sd = weights64(cfg, segmem_num_layers)
    for v in sd.values():
        v.grad = None
    loss, logits = oracle_loss(sd, cfg, mel, lab, variant, prev, max(1, segmem_num_layers), drop)
    loss.backward()
    return float(loss.item()), logits.detach(), {k: v.grad for k, v in sd.items()}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if b.norm() > 0 else float(a.norm())
