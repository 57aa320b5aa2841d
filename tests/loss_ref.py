"""TEST INFRASTRUCTURE ONLY: float64 restatement of the cross-entropy with label smoothing and z-loss (csrc/loss.hip
`ce_wave_kernel<., ., true>` / `ce_kernel<., true>`), next to tests/sample_ref.py.  Plain torch on the CPU;
nothing here shares code with the kernels.

Per scored row i (target t != -100), l the row's logits, lse = logsumexp(l), p = softmax(l), (w_i, n_i) the row's weights
((1, 1); with `weighted` (3, 2) for an instrument token in [inst_lo, inst_hi]; (0, 0) for an ignored row):

    nll_i = lse - l[t]
    u_i   = lse - mean_j l[j]
    r_i   = (1 - eps) * nll_i + eps * u_i + z * lse^2
    objective = sum_i w_i r_i / sum_i n_i
    nll       = sum_i w_i nll_i / sum_i n_i
    d objective / d l[j] = grad_scale * w_i / denom * (p_j (1 + 2 z lse) - (1 - eps) [j == t] - eps / V)
"""
import torch


def weights(targets, weighted=False, inst_lo=1135, inst_hi=1262):
    """(w, n) float64 per row."""
    scored = targets != -100
    inst = scored & (targets >= inst_lo) & (targets <= inst_hi) if weighted else torch.zeros_like(scored)
    w = torch.where(inst, 3.0, 1.0).double() * scored
    n = torch.where(inst, 2.0, 1.0).double() * scored
    return w, n


def objective(logits, targets, eps=0.0, z=0.0, weighted=False, inst_lo=1135, inst_hi=1262):
    """(objective, nll) as float64 0-d tensors, differentiable in `logits` (any float dtype; the arithmetic is float64)."""
    l = logits.double()
    w, n = weights(targets, weighted, inst_lo, inst_hi)
    lse = torch.logsumexp(l, dim=-1)
    t = targets.clamp(min=0)
    nll = lse - l.gather(1, t[:, None])[:, 0]
    u = lse - l.mean(dim=-1)
    r = (1.0 - eps) * nll + eps * u + z * lse * lse
    den = n.sum()
    return (w * r).sum() / den, (w * nll).sum() / den


def gradient(logits, targets, eps=0.0, z=0.0, weighted=False, inst_lo=1135, inst_hi=1262, grad_scale=1.0):
    """The closed-form d objective / d logits, float64 [rows, V]; the rows of ignored targets are zero."""
    l = logits.double()
    V = l.shape[1]
    w, n = weights(targets, weighted, inst_lo, inst_hi)
    lse = torch.logsumexp(l, dim=-1, keepdim=True)
    g = torch.exp(l - lse) * (1.0 + 2.0 * z * lse) - eps / V
    rows = torch.nonzero(targets != -100)[:, 0]
    g[rows, targets[rows]] -= 1.0 - eps
    return g * (grad_scale * w / n.sum())[:, None]


def inst_range(V):
    """The instrument-token range of a test vocabulary: the product's 1135..1262 where it fits, else a range of the same
    width (128 ids) below the top of the vocabulary, passed to the kernel as inst_lo / inst_hi."""
    return (1135, 1262) if V > 1262 else (V - 200, V - 73)


def case(rows, V, weighted, seed=0):
    """The logits and targets of the kernel tests: randn * 3, one row shifted by +80 and one by -80 (where lse^2 and the
    maximum subtraction go wrong in f32), every fifth target -100, the others uniform over the vocabulary and, with
    `weighted`, every odd row's inside the instrument range (both weights occur in one sum)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, V, generator=g) * 3
    logits[1] += 80.0
    logits[2] -= 80.0
    targets = torch.randint(0, V, (rows,), generator=g)
    if weighted:
        lo, hi = inst_range(V)
        targets[1::2] = torch.randint(lo, hi + 1, (len(targets[1::2]),), generator=g)
    targets[::5] = -100
    return logits, targets
