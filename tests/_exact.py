"""Constructions and checkers of the element-exact kernel tests (tests/test_exact_gpu.py; proven on the CPU by
tests/test_exact_constructions_cpu.py).  Plain torch on whatever device the tensors live on; nothing here touches the library.

A. GEMM operands are small integers, so every product and every partial sum in any order is an integer below 2^24 and the f32
   result does not depend on the summation order: the kernels must return the float64 matmul bit for bit.
B. `attention_case` builds attention inputs whose softmax is saturated onto one or two keys per query: O, LSE, dQ, dK and dV
   are known in closed form at every element, every nonzero step of an output is at least 1/2.
C. `row_errors` scores a Gaussian-input result per 64-wide row instead of per tensor; `attention_rounded` is the fp64
   restatement with the kernels' rounding points that sets the limit.
"""
import functools

import torch

# ---- A. integer GEMMs --------------------------------------------------------------------------------------------------------

INT_LO, INT_HI = -3, 3                  # operands
C0_LO, C0_HI = -100, 100                # what an accumulate case starts from
EXACT_F32 = 2 ** 24                     # every integer of magnitude <= 2^24 is an f32

NT_SHAPES = [(1, 8, 32), (129, 136, 96), (1000, 1152, 512), (2047, 392, 480), (2048, 392, 480), (2049, 392, 480),
             (4097, 512, 1024), (130, 2048, 512), (3072, 512, 2048), (3000, 512, 2304), (65536, 512, 1024)]
NT_SPLITK_SHAPES = [(3072, 512, 2048), (3000, 512, 2304)]
NT_STRIDED = (300, 1152, 384, 768, 512)          # A = columns 384:768 of a [300, 1152] buffer, N = 512
# the f32-input case whose operands no bf16 holds: |a| < 2^11 (12-bit integers), |b| < 2^8, K = 32
NT_F32_WIDE = dict(M=129, N=136, K=32, a_max=2047, b_max=255)
TN_SHAPES = [(64, 72, 40), (1000, 512, 384), (4096, 1152, 512), (8200, 896, 320), (32768, 512, 520), (34773, 696, 1008),
             (65536, 1152, 512)]
TN_GROUP_SITES = [(1100, 384, 320), (3000, 1152, 512), (4097, 256, 576), (2048, 640, 256)]      # ragged token counts
TN_F32_SHAPES = [(64, 72, 40), (1000, 512, 384), (4096, 1152, 512), (8200, 896, 320)]


def int_sum_bound(depth, a_max=max(-INT_LO, INT_HI), b_max=max(-INT_LO, INT_HI), c0_max=max(-C0_LO, C0_HI)):
    """Largest magnitude any partial sum of `depth` products (plus the accumulate start) can reach."""
    return depth * a_max * b_max + c0_max


def rand_ints(shape, lo, hi, dtype, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device=device, generator=g, dtype=torch.int32).to(dtype)


def assert_equal_everywhere(got, want, what):
    """torch.equal on the whole tensor, with the coordinates of the first differing elements in the message."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:8]]
    raise AssertionError("%s: %d of %d elements differ; (index, got, want) of the first: %s" % (what, idx.shape[0], got.numel(), first))


def rel_l2(a, b):
    """The whole-tensor figure the older kernel tests bound (tests/test_kernels_gpu.py `_rel`)."""
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


# ---- B. attention with closed forms ----------------------------------------------------------------------------------------------

HD, CODE, GAIN = 64, 56, 2              # head dim; dims 0..55 carry the code; queries are GAIN x the selected key's code
MIN_MARGIN = 40.0                       # nats between a selected score and every other: leakage exp(-40) < 1e-17
ATTN_TOL = 1.0 / 8                      # absolute, per element (every real fault moves an element by >= 1/2)
LSE_RTOL = 1e-4

ATTN_SHAPES = [(1, 1, 1, 1, False), (1, 1, 33, 33, True), (1, 2, 129, 257, False), (2, 3, 200, 72, False),
               (1, 2, 300, 300, True), (2, 6, 256, 256, False), (1, 3, 1000, 300, False), (1, 6, 1024, 320, False),
               (1, 6, 64, 1024, False), (1, 1, 1088, 1088, True), (22, 6, 1024, 1024, True)]
VARLEN_LENGTHS = [0, 37, 300, 1]
VARLEN_L, VARLEN_CROSS_KEYS = 320, 320
ROW_BOUND_SHAPES = [(2, 3, 200, 72, False), (1, 2, 300, 300, True), (2, 6, 256, 256, False), (1, 6, 1024, 320, False),
                    (1, 1, 1088, 1088, True)]
ROW_BOUND_FACTOR = 4.0


def onepass_takes(Lq, Lk, causal):
    """Shapes the one-pass backward admits once MRMT3_ATTN_ONEPASS_MIN_BH=1 lifts its batch threshold (attention_onepass.hip)."""
    return (not causal) and Lq >= 32 and 256 <= Lk <= 320


def _pm1(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).double() * 2 - 1


@functools.lru_cache(maxsize=None)
def codebook(n_codes, seed=0, gain=GAIN):
    """n_codes random +-1 codes of CODE dims whose pairwise dot products leave a margin of >= MIN_MARGIN nats between
    gain * CODE (a query against its own code) and gain * dot (against any other).  Returns (codes [n, CODE] fp64, margin)."""
    for attempt in range(256):
        gen = torch.Generator().manual_seed(100003 * seed + 1009 * n_codes + attempt)
        c = _pm1((n_codes, CODE), gen)
        d = c @ c.t()
        d.fill_diagonal_(-CODE)
        margin = gain * (CODE - d.max().item()) if n_codes > 1 else float("inf")
        if margin >= MIN_MARGIN:
            return c, margin
    raise AssertionError("no code book of %d codes with a margin of %g nats" % (n_codes, MIN_MARGIN))


def attention_head(Lq, Lk, causal, gen, gain=GAIN):
    """One (batch, head): q [Lq, 64], k / v [Lk, 64], d_o [Lq, 64] and the closed forms o, lse, dq, dk, dv (all fp64), plus
    `margin`, the least gap in nats between a selected score and any other visible one."""
    book, margin = codebook((Lk + 1) // 2)
    perm = torch.randperm(Lk, generator=gen)                       # code c sits on keys perm[2c], perm[2c + 1]
    code_of = torch.empty(Lk, dtype=torch.long)
    code_of[perm] = torch.arange(Lk) // 2
    mate = torch.full((Lk,), -1, dtype=torch.long)
    ev, od = perm[0:2 * (Lk // 2):2], perm[1::2]
    mate[ev], mate[od] = od, ev
    codes = (book * _pm1((1, CODE), gen))[code_of]                 # (a column sign flip keeps every dot product)
    tail = _pm1((Lk, HD - CODE), gen)
    same = (tail[ev] == tail[od]).all(1)
    tail[ev[same], 0] *= -1                                        # the two keys of a pair differ in dims 56..63
    k = torch.cat([codes, tail], 1)
    i = torch.arange(Lq)
    if causal:
        pi = (torch.rand(Lq, generator=gen, dtype=torch.float64) * (torch.clamp(i, max=Lk - 1) + 1)).long()
        pi = torch.minimum(pi, torch.clamp(i, max=Lk - 1))
    else:
        pi = torch.randint(0, Lk, (Lq,), generator=gen)
    q = torch.cat([gain * codes[pi], torch.zeros(Lq, HD - CODE, dtype=torch.float64)], 1)
    v = torch.randint(-1, 2, (Lk, HD), generator=gen).double()
    d_o = torch.randint(-1, 2, (Lq, HD), generator=gen).double()

    a, b = pi, mate[pi]
    vis = (b >= 0) & ((b <= i) if causal else torch.ones(Lq, dtype=torch.bool))
    bb = b.clamp(min=0)
    visf = vis.double()[:, None]
    n = 1.0 + vis.double()
    o = (v[a] + visf * v[bb]) / n[:, None]
    lse = gain * CODE + torch.log(n)
    dv = torch.zeros(Lk, HD, dtype=torch.float64)
    dv.index_add_(0, a, d_o / n[:, None])
    dv.index_add_(0, bb, visf * d_o / n[:, None])
    ds_a = vis.double() * ((d_o * v[a]).sum(1) - (d_o * v[bb]).sum(1)) / 4          # dS on key a; -ds_a on its mate
    dk = torch.zeros(Lk, HD, dtype=torch.float64)
    dk.index_add_(0, a, ds_a[:, None] * q)
    dk.index_add_(0, bb, -ds_a[:, None] * q)
    dq = ds_a[:, None] * (k[a] - k[bb])
    return dict(q=q, k=k, v=v, d_o=d_o, o=o, lse=lse, dq=dq, dk=dk, dv=dv, margin=margin, pi=pi, mate=mate)


class AttnCase:
    """Inputs q, k, v, d_o as [B*L, H*64] f32 tensors (every value a bf16) and the closed forms o, dq, dk, dv in the same
    layout, lse [B, H, Lq]; `margin` in nats.  CPU tensors; shared between tests, never modified."""
    names = ("q", "k", "v", "d_o", "o", "dq", "dk", "dv")


def _assemble(heads, B, H, Lq, Lk):
    c = AttnCase()
    c.B, c.H, c.Lq, c.Lk = B, H, Lq, Lk
    for name in AttnCase.names:
        L = Lk if name in ("k", "v", "dk", "dv") else Lq
        t = torch.stack([torch.stack([heads[b][h][name] for h in range(H)], 1) for b in range(B)])     # [B, L, H, 64]
        setattr(c, name, t.reshape(B * L, H * HD).float())
    c.lse = torch.stack([torch.stack([heads[b][h]["lse"] for h in range(H)]) for b in range(B)])          # fp64
    c.margin = min(hd["margin"] for row in heads for hd in row)
    assert c.margin >= MIN_MARGIN, c.margin
    for name in ("o", "dq", "dk", "dv"):                     # a bf16 output can hold every expected value exactly
        t = getattr(c, name)
        assert torch.equal(t.bfloat16().float(), t), (name, t.abs().max().item())
    return c


@functools.lru_cache(maxsize=2)
def attention_case(B, H, Lq, Lk, causal, seed=0):
    gen = torch.Generator().manual_seed(7919 * seed + 31 * Lq + Lk + (1 if causal else 0))
    heads = [[attention_head(Lq, Lk, causal, gen) for _ in range(H)] for _ in range(B)]
    c = _assemble(heads, B, H, Lq, Lk)
    c.causal = causal
    return c


@functools.lru_cache(maxsize=2)
def varlen_case(lengths, H, cross_keys, seed=0):
    """Packed rows of `lengths` tokens.  cross_keys = 0: causal self-attention, k / v packed like q.  Otherwise every row
    attends to its own `cross_keys` dense keys, not causal.  Returns an AttnCase whose q-side tensors are [T, H*64] with
    T = sum(lengths) (the caller pads to Tcap) and lse [H, T]; k-side tensors are [T, H*64] or [B*cross_keys, H*64]."""
    gen = torch.Generator().manual_seed(104729 * seed + 17 * sum(lengths) + cross_keys)
    c = AttnCase()
    c.H, c.lengths, c.margin = H, lengths, float("inf")
    parts = {n: [] for n in AttnCase.names + ("lse",)}
    for n_tok in lengths:
        Lk = cross_keys if cross_keys else n_tok
        if Lk == 0:
            continue
        heads = [attention_head(n_tok, Lk, cross_keys == 0, gen) for _ in range(H)]
        for name in AttnCase.names:
            parts[name].append(torch.stack([hd[name] for hd in heads], 1).reshape(-1, H * HD).float())
        parts["lse"].append(torch.stack([hd["lse"] for hd in heads]))                      # [H, n_tok] fp64
        c.margin = min(c.margin, min(hd["margin"] for hd in heads))
    for name in AttnCase.names:
        setattr(c, name, torch.cat(parts[name]))
    c.lse = torch.cat(parts["lse"], 1)
    assert c.margin >= MIN_MARGIN, c.margin
    return c


def _heads(x, B, L, H):
    return x.reshape(B, L, H, HD).permute(0, 2, 1, 3)


def _rows(xh, B, L, H):
    return xh.permute(0, 2, 1, 3).reshape(B * L, H * HD)


def _mask(Lq, Lk, causal, device, unmask=()):
    m = torch.zeros(Lq, Lk, dtype=torch.bool, device=device)
    if causal:
        m = torch.arange(Lk, device=device)[None, :] > torch.arange(Lq, device=device)[:, None]
    for i, j in unmask:
        m[i, j] = False
    return m


def attention_autograd(q, k, v, d_o, B, H, Lq, Lk, causal, unmask=()):
    """fp64 softmax(q k^T) v (T5: no 1/sqrt(d)) and its autograd: (o, lse [B, H, Lq], dq, dk, dv), row layouts as given.
    `unmask`: (query, key) pairs made visible against the causal rule (the checker-sensitivity tests)."""
    qr, kr, vr = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    s = _heads(qr, B, Lq, H) @ _heads(kr, B, Lk, H).transpose(2, 3)
    s = s.masked_fill(_mask(Lq, Lk, causal, s.device, unmask), float("-inf"))
    o = _rows(torch.softmax(s, -1) @ _heads(vr, B, Lk, H), B, Lq, H)
    o.backward(d_o.double())
    return o.detach(), torch.logsumexp(s.detach(), -1), qr.grad, kr.grad, vr.grad


def _bf16(x):
    return x.float().bfloat16().double()


def attention_rounded(q, k, v, d_o, B, H, Lq, Lk, causal):
    """The fp64 restatement with the bf16 kernels' documented rounding points, placed where the kernels place them
    (csrc/attention.hip): the forward rounds exp(s - rowmax) to bf16 before P V and normalises by the unrounded sum; the
    backward rounds P = exp(s - lse) to bf16 before P^T dO, forms dS = P (dP - delta) from the unrounded P with
    delta = rowsum(dO * O) of the forward's unrounded output, and rounds dS to bf16 before dS K and dS^T Q; the outputs are
    rounded to bf16.  Everything else is fp64.  Returns (o, dq, dk, dv)."""
    qh, kh, vh, gh = (_heads(t.double(), B, L, H) for t, L in ((q, Lq), (k, Lk), (v, Lk), (d_o, Lq)))
    s = qh @ kh.transpose(2, 3)
    s = s.masked_fill(_mask(Lq, Lk, causal, s.device), float("-inf"))
    pt = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (_bf16(pt) @ vh) / pt.sum(-1, keepdim=True)
    p = torch.softmax(s, -1)
    dv = _bf16(p).transpose(2, 3) @ gh
    delta = (gh * o).sum(-1, keepdim=True)
    ds = _bf16(p * (gh @ vh.transpose(2, 3) - delta))
    dq = ds @ kh
    dk = ds.transpose(2, 3) @ qh
    return tuple(_bf16(_rows(t, B, L, H)) for t, L in ((o, Lq), (dq, Lq), (dk, Lk), (dv, Lk)))


def max_deviation(got, want):
    """(max |got - want|, flat index of it); a NaN or Inf anywhere counts as an infinite deviation at its place."""
    d = (got.double() - want.double().to(got.device)).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    i = int(d.reshape(-1).argmax())
    return float(d.reshape(-1)[i]), i


def check_elements(name, got, want, tol, H=None):
    """Every element of `got` within `tol` (absolute) of `want`; returns the largest deviation.  The message names the
    element: (row, head, dim) for a [rows, H*64] tensor."""
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    dev, i = max_deviation(got, want)
    if not dev <= tol:
        cols = got.shape[-1]
        where = (i // cols, (i % cols) // HD, i % HD) if H else i
        n_bad = int(((got.double() - want.double().to(got.device)).abs() > tol).sum())
        raise AssertionError("%s: max deviation %.4g > %.4g at (row, head, dim) = %s: got %.6g, want %.6g; %d elements out" % (
            name, dev, tol, where, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]), n_bad))
    return dev


def check_lse(name, got, want, rtol=LSE_RTOL):
    dev, i = max_deviation(got / want.to(got.device), torch.ones_like(want))
    assert dev <= rtol, "%s: max relative deviation %.4g > %.4g at flat index %d" % (name, dev, rtol, i)
    return dev


# ---- C. per-row bound on Gaussian inputs -------------------------------------------------------------------------------------------

def row_errors(got, ref, H):
    """e_r = |got_r - ref_r| / max(|ref_r|, 1e-3 * median row norm of the tensor) for every 64-wide row of every head:
    [rows, H] fp64.  Rows with a near-zero reference are compared absolutely; no row is left out."""
    rows = got.shape[0]
    g, r = got.double().reshape(rows, H, HD), ref.double().to(got.device).reshape(rows, H, HD)
    rn = r.norm(dim=-1)
    e = (g - r).norm(dim=-1) / torch.maximum(rn, 1e-3 * rn.median())
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def gaussian_attention_inputs(B, H, Lq, Lk, device):
    """The inputs of tests/test_kernels_gpu.py::test_attn_bwd_bf16 (same seed, same draws): bf16 q, k, v, d_o."""
    g = torch.Generator(device="cpu").manual_seed(Lq * 3 + Lk)
    q = (torch.randn(B * Lq, H * HD, generator=g) * 0.35).to(device).bfloat16()
    k = torch.randn(B * Lk, H * HD, generator=g).to(device).bfloat16()
    v = torch.randn(B * Lk, H * HD, generator=g).to(device).bfloat16()
    d_o = torch.randn(B * Lq, H * HD, generator=g).to(device).bfloat16()
    return q, k, v, d_o
