"""Constructions and checkers of the element-exact tests of the KV-cached decode step (csrc/decode.hip): probe decoders.
Proven on the CPU by tests/test_exact_decode_cpu.py, run on the device by tests/test_exact_decode_gpu.py.  Plain torch;
nothing here touches the library.

A probe is a ONE-layer decoder (H = 6, d_ff = 1024) whose weights, cross K/V and per-step inputs x0[b][t] (fed as prefix rows
with a zero position table) are chosen so that a step's logits show one kernel's output at every element:

  * every x0 entry is +-1, so mean(x^2) = 1 exactly and rstd = rsqrt(1 + eps) is within 1e-6 of 1; norm weights are small
    bf16-exact integers, so a bf16 handle rounds a normed activation to exactly +-lnw[k] (an f32 handle gives the same
    integer times (1 - 5e-7)); 0/1 or small-integer projection weights then give f32-exact sums in any order;
  * a zero output projection takes a sublayer out of the residual stream; with lm_head = identity (V = 512) and final_ln = 1
    the logits are the normalised final residual, and a dimension nothing writes (the pilot, x = +-1) gives the scale back.

1  self_attention_probe    dec_attn over the cache (len = t + 1) and the fused q|k|v projection (MODE 1)
2  cross_attention_probe   dec_attn at a fixed length over the caller's K|V buffer, the q projection (MODE 0)
   q_cross_probe           that q projection (N = 384) at unsaturated integer scores, where a wrong q element shows
   q_self_probe            the same for the q rows of q|k|v and for the softmax over the cache
3  lm_head_probe           MODE 0 with integer operands at a ragged vocabulary
4  res_inner_probe / res_ff_probe   the two residual projections (K = 384, K = 1024) with sparse +-1 weights
5  geglu_probe             MODE 2: gelu_new(h0) * h1 on exact integer h0, h1

`forward` is the one-layer step written once: in float64 it is the reference (bf16 = True places the kernels' rounding points),
in float32 with a `fault` it is the emulation the CPU proof uses to show that each checker resolves each fault."""
import math
from types import SimpleNamespace

import torch

import _exact as ex

D, H, HD, INNER, DFF = 512, 6, 64, 384, 1024
CODE, GAIN = ex.CODE, ex.GAIN
EPS = 1e-6
U = 2.0 ** -24                          # unit roundoff of f32
READ = 4                                # a readout projection puts READ * o[j] onto a residual dimension
X_MAX = 32                              # construction condition of the residual probes: |x| <= X_MAX at every element
TIE_REL = 2.0 ** -20                    # a g within TIE_REL * |g| (or within its own f32 error) of a bf16 tie gets the widened bound
WIDE_CAP = 0.01                         # at most this share of a GEGLU probe's logits may get the widened bound

F64 = torch.float64

# the shapes the device tests run (tests/test_exact_decode_gpu.py); the CPU proof builds the same probes
SELF_LEN = 1024                         # n_prefix of probe 1: len runs through 1..1024
ENC_LENS = (1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1001, 2112)
CROSS_STEPS = 64
VOCABS = (1536, 1491)
SHORT_STEPS = 16                        # positions of probes 3 to 5
RES_ENC_LEN = 33


def _pm1(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).double() * 2 - 1


def _bf16(t):
    return t.float().bfloat16().to(t.dtype)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * (x * x * x))))


# ---- the probe record ------------------------------------------------------------------------------------------------------------

def _base(B, T, gen, V=D, Lc=1):
    """All sublayers switched off: zero projections, unit norms, identity lm_head, x0 = +-1, a zero cross K|V of one key."""
    p = SimpleNamespace(B=B, T=T, V=V, Lc=Lc)
    z = lambda *s: torch.zeros(*s, dtype=F64)
    p.w = dict(ln_self=torch.ones(D, dtype=F64), w_qkv=z(3 * INNER, D), w_o_self=z(D, INNER),
               ln_cross=torch.ones(D, dtype=F64), w_q_cross=z(INNER, D), w_o_cross=z(D, INNER),
               ln_ff=torch.ones(D, dtype=F64), w_wi=z(2 * DFF, D), w_wo=z(D, DFF),
               final_ln=torch.ones(D, dtype=F64), lm_head=torch.eye(D, dtype=F64) if V == D else z(V, D))
    p.x0 = _pm1((B, T, D), gen)
    p.ck, p.cv = z(B, Lc, INNER), z(B, Lc, INNER)
    return p


def check_probe(p):
    """What every construction relies on: +-1 inputs and operands a bf16 holds."""
    assert bool((p.x0.abs() == 1).all())
    for name, t in list(p.w.items()) + [("ck", p.ck), ("cv", p.cv)]:
        assert torch.equal(_bf16(t), t), name


def state_dict(p):
    """The probe as a `oracle.t5_ref.decode_step_logits` state dict and config (no token is ever embedded)."""
    w, b = p.w, "decoder.block.0.layer"
    sd = {"decoder_embed_tokens.weight": torch.zeros(1, D, dtype=F64), "lm_head.weight": w["lm_head"],
          "decoder.final_layer_norm.weight": w["final_ln"], f"{b}.0.layer_norm.weight": w["ln_self"],
          f"{b}.1.layer_norm.weight": w["ln_cross"], f"{b}.2.layer_norm.weight": w["ln_ff"],
          f"{b}.0.SelfAttention.o.weight": w["w_o_self"], f"{b}.1.EncDecAttention.q.weight": w["w_q_cross"],
          f"{b}.1.EncDecAttention.o.weight": w["w_o_cross"], f"{b}.2.DenseReluDense.wi_0.weight": w["w_wi"][:DFF],
          f"{b}.2.DenseReluDense.wi_1.weight": w["w_wi"][DFF:], f"{b}.2.DenseReluDense.wo.weight": w["w_wo"]}
    for j, n in enumerate("qkv"):
        sd[f"{b}.0.SelfAttention.{n}.weight"] = w["w_qkv"][j * INNER:(j + 1) * INNER]
    cfg = dict(num_heads=H, layer_norm_epsilon=EPS, num_decoder_layers=1)
    return sd, cfg


# ---- the one-layer step ------------------------------------------------------------------------------------------------------------
# Faults (the emulation only): "drop_last_key" (the last key when len % 256 == 1), "ignore_512" (keys >= 512), "v_next" (V row k
# read as k + 1), "other_head_k" / "other_head_v", "swap_rows" (cache rows of sequences 0 and 1), "k_prev" (K written to
# position t - 1), ("skip_kblock", projection, first column[, in the first n rows only]), "wi_pair" (row n with n + N - 1), ("seq16", projection) (sequence
# 16 from sequence 15's activations), "lm_last_twice" / "lm_last_skipped" (output row N - 1).
PROJECTIONS = ("qkv", "o_self", "q_cross", "o_cross", "wi", "wo", "lm_head")


def _attend(q, k, v, causal, fault):
    """q [B, H, T, 64], k / v [B, H, L, 64] -> softmax(q k^T) v [B, H, T, 64]; step t of a causal call sees keys 0..t."""
    T, L = q.shape[2], k.shape[2]
    if fault == "other_head_k":
        k = k.roll(1, 1)
    if fault == "other_head_v":
        v = v.roll(1, 1)
    if fault == "v_next":
        v = v.roll(-1, 2)
    key = torch.arange(L)[None, :]
    n = torch.arange(1, T + 1)[:, None] if causal else torch.full((T, 1), L)
    hide = key >= n
    if fault == "drop_last_key":
        hide = hide | ((key == n - 1) & (n % 256 == 1) & (n > 1))
    if fault == "ignore_512":
        hide = hide | (key >= 512)
    if causal and fault == "k_prev":                         # row j holds the key of step j + 1; row t is still empty at step t
        sc = q @ k.roll(-1, 2).transpose(2, 3)
        sc = sc.masked_fill(key == n - 1, 0.0)
    else:
        sc = q @ k.transpose(2, 3)
    return torch.softmax(sc.masked_fill(hide, float("-inf")), -1) @ v


def forward(p, bf16, dtype=F64, fault=None):
    """The step of csrc/decode.hip for every (row, position) of the probe at once (the inputs of every step are known, so a
    causal mask stands for the cache).  `bf16`: round where a bf16 handle rounds: the normed activation entering a projection,
    the K/V cache entries, the attention and gated-GELU outputs entering their projections.  Returns the residual before
    the final norm `x`, the unrounded normed residual `v`, `logits`, and `o_self`, `o_cross`, `h0`, `h1`, `g`."""
    rnd = _bf16 if bf16 else (lambda t: t)
    W = {k: t.to(dtype) for k, t in p.w.items()}
    B, T = p.B, p.T
    fname = fault[0] if isinstance(fault, tuple) else fault

    def norm(x, lnw):
        return rnd(lnw * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS)))

    def proj(name, a, Wm):
        if fname == "skip_kblock" and fault[1] == name:
            Wm = Wm.clone()
            Wm[:(fault[3] if len(fault) > 3 else None), fault[2]:fault[2] + 32] = 0
        if fname == "seq16" and fault[1] == name and B > 16:
            a = a.clone()
            a[16] = a[15]
        return a @ Wm.t()

    heads = lambda t: t.reshape(B, -1, H, HD).transpose(1, 2)
    rows = lambda t: t.transpose(1, 2).reshape(B, T, INNER)
    r = SimpleNamespace()
    x = p.x0.to(dtype)
    q, k, v = proj("qkv", norm(x, W["ln_self"]), W["w_qkv"]).split(INNER, -1)
    k, v = rnd(k), rnd(v)
    if fname == "swap_rows":
        idx = torch.arange(B)
        idx[0], idx[1] = 1, 0
        k, v = k[idx], v[idx]
    r.o_self = rows(_attend(heads(q), heads(k), heads(v), True, fname))
    x = x + proj("o_self", rnd(r.o_self), W["w_o_self"])
    q = proj("q_cross", norm(x, W["ln_cross"]), W["w_q_cross"])
    r.o_cross = rows(_attend(heads(q), heads(p.ck.to(dtype)), heads(p.cv.to(dtype)), False, fname))
    x = x + proj("o_cross", rnd(r.o_cross), W["w_o_cross"])
    h = proj("wi", norm(x, W["ln_ff"]), W["w_wi"])
    r.h0, r.h1 = h[..., :DFF], h[..., DFF:]
    if fname == "wi_pair":
        r.h1 = r.h1.roll(1, -1)
    r.g = rnd(gelu_new(r.h0) * r.h1)
    r.x = x + proj("wo", r.g, W["w_wo"])
    r.rstd = torch.rsqrt((r.x * r.x).mean(-1, keepdim=True) + EPS)
    r.v = W["final_ln"] * (r.x * r.rstd)
    r.logits = proj("lm_head", rnd(r.v), W["lm_head"])
    if fname == "lm_last_skipped":                           # the row keeps what the step before left there
        r.logits = r.logits.clone()
        r.logits[:, 1:, -1] = r.logits[:, :-1, -1].clone()
        r.logits[:, 0, -1] = 0
    if fname == "lm_last_twice":                             # the second write lands one element on: the next sequence's row 0
        r.logits = r.logits.clone()
        r.logits[1:, :, 0] = r.logits[:-1, :, -1].clone()
    return r


def emulate(p, bf16, fault=None):
    """The f32 emulation of the step (bf16 at the kernels' rounding points), optionally with one fault: logits [B, T, V] f32."""
    return forward(p, bf16, torch.float32, fault).logits


# ---- checkers --------------------------------------------------------------------------------------------------------------------

def check_within(what, got, ref, bound):
    """Every element of `got` [B, T, N] within `bound` (scalar or tensor, absolute) of `ref`; returns the largest
    error / bound.  A failure names the first offending (row, step, element)."""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    err = (got.double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    bad = ~(ratio <= 1)
    if bool(bad.any()):
        idx = bad.nonzero()
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx[:6]]
        raise AssertionError("%s: %d of %d elements out of bound; (row, step, element), got, want, bound of the first: %s" % (
            what, idx.shape[0], err.numel(), first))
    return float(ratio.max())


def check_equal(what, got, want):
    """Bit-for-bit equality of [B, T, N] tensors, the first differing (row, step, element) in the message."""
    ex.assert_equal_everywhere(got, want.to(got.dtype), what + " (row, step, element)")


def decode_o(p, logits):
    """The attention output [B, T, 384] a readout probe's logits show: x = logits / |pilot logit|, o = (x - x0) / READ."""
    lg = logits.double()
    x = lg / lg[..., p.pilot].abs()[..., None]
    return (x[..., p.readout] - p.x0[..., p.readout]) / READ


def check_attention(p, logits, what):
    """Probes 1 and 2: the decoded o against the closed form at every (row, step, head * 64 + dim), within ex.ATTN_TOL."""
    return check_within(what, decode_o(p, logits), p.o_want, ex.ATTN_TOL)


# ---- 1. self-attention over the cache -----------------------------------------------------------------------------------------------

def _select(v, pi, mate, visible):
    """Closed form of a saturated softmax: query t sits on key pi[t] and, where visible, on that key's mate."""
    m = mate[pi]
    vis = ((m >= 0) & visible(m)).double()[:, None]
    return (v[pi] + vis * v[m.clamp(min=0)]) / (1.0 + vis)


def _readout(p, name, dims):
    p.readout = dims
    p.w[name][dims, torch.arange(INNER)] = READ


def self_attention_probe(B, L, seed=0):
    """x0[b][t] carries step t's query code (56 dims, ln_self = GAIN there), key row (64 dims) and value rows (6 x 64 dims);
    8 dims are spare, one of them the pilot.  w_qkv is a 0/1 selection with a signed permutation of the code dims per head
    (applied to q and k alike: the scores are every head's, another head's K scrambles them).  Keys and queries of a row
    are `ex.attention_head(L, L, causal=True)`'s, one independent draw per row; the step whose length is 1 mod 256 asks for
    its own newest key.  w_o_self reads READ * o onto 384 dims; w_o_cross = w_wo = 0."""
    gen = torch.Generator().manual_seed(52361 * seed + 977 * L + B)
    p = _base(B, L, gen)
    dims = torch.randperm(D, generator=gen)
    qd, kd, vd, p.pilot = dims[:CODE], dims[CODE:CODE + HD], dims[120:504], int(dims[504])
    ar = torch.arange(CODE)
    for h in range(H):
        perm, sign = torch.randperm(CODE, generator=gen), _pm1((CODE,), gen)
        p.w["w_qkv"][h * HD + ar, qd[perm]] = sign
        p.w["w_qkv"][INNER + h * HD + ar, kd[perm]] = sign
        p.w["w_qkv"][INNER + h * HD + torch.arange(CODE, HD), kd[CODE:]] = 1
    p.w["w_qkv"][2 * INNER + torch.arange(INNER), vd] = 1
    p.w["ln_self"][qd] = GAIN
    _readout(p, "w_o_self", dims[:INNER])
    t = torch.arange(L)
    p.margin, o = float("inf"), []
    for b in range(B):
        hd = ex.attention_head(L, L, True, gen)
        pi = hd["pi"].clone()
        own = (t % 256 == 0) | (t % 97 == 5)                 # these steps select the key they have just appended
        pi[own] = t[own]
        p.x0[b][:, kd] = hd["k"]
        p.x0[b][:, qd] = hd["k"][pi, :CODE]
        o.append(_select(p.x0[b][:, vd], pi, hd["mate"], lambda m: m <= t))
        p.margin = min(p.margin, hd["margin"])
    p.o_want = torch.stack(o)
    assert p.margin >= ex.MIN_MARGIN
    return p


# ---- 2. cross-attention ---------------------------------------------------------------------------------------------------------------

def cross_attention_probe(B, T, Lc, seed=0, gen=None):
    """K / V of every (row, head) are an independent `ex.attention_head(., Lc, causal=False)` draw in the caller's K|V buffer;
    x0 carries 6 x 56 query-code dims (ln_cross = GAIN there, w_q_cross a 0/1 selection).  Step 0 asks for the last key, step
    1 for key 0, the others for a random one.  w_o_cross reads READ * o onto 384 dims; the self-attention sublayer is zero."""
    gen = gen or torch.Generator().manual_seed(60013 * seed + 131 * Lc + 7 * T + B)
    p = _base(B, T, gen, Lc=Lc)
    dims = torch.randperm(D, generator=gen)
    qd, p.pilot = dims[:H * CODE], int(dims[-1])
    ar = torch.arange(CODE)
    for h in range(H):
        p.w["w_q_cross"][h * HD + ar, qd[h * CODE + ar]] = 1
    p.w["ln_cross"][qd] = GAIN
    _readout(p, "w_o_cross", dims[64:64 + INNER])
    p.margin = float("inf")
    p.o_want = torch.zeros(B, T, INNER, dtype=F64)
    for b in range(B):
        for h in range(H):
            hd = ex.attention_head(1, Lc, False, gen)
            pi = torch.randint(0, Lc, (T,), generator=gen)
            pi[0] = Lc - 1
            if T > 1:
                pi[1] = 0
            sl = slice(h * HD, (h + 1) * HD)
            p.ck[b][:, sl], p.cv[b][:, sl] = hd["k"], hd["v"]
            p.x0[b][:, qd[h * CODE + ar]] = hd["k"][pi, :CODE]
            p.o_want[b][:, sl] = _select(hd["v"], pi, hd["mate"], lambda m: torch.ones_like(m, dtype=torch.bool))
            p.margin = min(p.margin, hd["margin"])
    assert p.margin >= ex.MIN_MARGIN
    return p


def q_cross_probe(B, T, seed=0):
    """The cross-attention q projection where a saturated softmax cannot hide it.  Probe 2's queries win by >= MIN_MARGIN
    nats, so a q that lost a 32-wide k-block still selects the same key.  Here w_q_cross is sparse in {-1, 0, 1} (every input
    dim covered by 2 rows, ln_cross = 1: q holds small integers), each of the 3 keys of a (row, head) has 3 entries +-1 and
    V is +-1: the scores are small exact integers, the softmax is NOT saturated, and a q element off by one moves o by a
    large multiple of the bound.  The reference is the float64 restatement; w_o_cross reads READ * o onto 384 dims."""
    gen = torch.Generator().manual_seed(110017 * seed + B)
    p = _base(B, T, gen, Lc=3)
    p.w["w_q_cross"] = _sparse_rows(INNER, D, 2, gen)
    _readout(p, "w_o_cross", torch.randperm(D, generator=gen)[:INNER])
    for b in range(B):
        for h in range(H):
            for j in range(p.Lc):
                c = h * HD + torch.randperm(HD, generator=gen)[:3]
                p.ck[b, j, c] = _pm1((3,), gen)
    p.cv = _pm1((B, p.Lc, INNER), gen)
    return p


def q_self_probe(B, T, seed=0):
    """The same for the q rows of the fused q|k|v projection and for dec_attn over the cache: the q rows of w_qkv are sparse
    in {-1, 0, 1}; every k row selects one of 128 input dims where ln_self = 1/4 (exact in bf16 like the integers), so a key
    is +-1/4 at all 64 dims and every q element moves every score; the v rows select an input dim each.  The softmax over
    keys 0..t is not saturated, so its normalisation is under test too."""
    gen = torch.Generator().manual_seed(120011 * seed + B)
    p = _base(B, T, gen)
    kin = torch.randperm(D, generator=gen)[:128]
    p.w["ln_self"][kin] = 0.25
    p.w["w_qkv"][:INNER] = _sparse_rows(INNER, D, 2, gen)
    r = torch.arange(INNER)
    p.w["w_qkv"][INNER + r, kin[torch.randint(0, 128, (INNER,), generator=gen)]] = _pm1((INNER,), gen)
    p.w["w_qkv"][2 * INNER + r, torch.randperm(D, generator=gen)[:INNER]] = _pm1((INNER,), gen)
    _readout(p, "w_o_self", torch.randperm(D, generator=gen)[:INNER])
    return p


def soft_bound(p, fw, bf16, side):
    """Probes with an unsaturated softmax (`side`: "cross" or "self").  A score is <= 64 fused multiply-adds of operands off
    by <= 8 u (an f32 handle's q and k): |ds| <= 72 u S, S = sum_d |q_d| |k_d|; p_j = exp(s_j - max) / sum moves by <= p_j (2
    max|ds| + 4 u of expf + 8 u of the sum and the division), and o, a combination of +-1 with those weights over <= 16 keys,
    by <= 2 * 72 u max S + 64 u (the P V sums included).  A bf16 handle then rounds o to bf16, where an f32 error can cross
    a tie: + one bf16 ulp of o."""
    if side == "cross":
        q, k, o, name = (p.x0 * p.w["ln_cross"]) @ p.w["w_q_cross"].t(), p.ck, fw.o_cross, "w_o_cross"
    else:
        q, k = ((p.x0 * p.w["ln_self"]) @ p.w["w_qkv"].t()).split(INNER, -1)[:2]
        o, name = fw.o_self, "w_o_self"
    assert k.shape[1] <= 16
    qa = q.abs().reshape(p.B, p.T, H, HD).transpose(1, 2)
    ka = k.abs().reshape(p.B, -1, H, HD).transpose(1, 2)
    smax = (qa @ ka.transpose(2, 3)).max(-1).values                                   # [B, H, T] (every key, visible or not)
    do = (U * (144 * smax + 64)).transpose(1, 2)[..., None].expand(p.B, p.T, H, HD).reshape(p.B, p.T, INNER)
    if bf16:
        do = do + torch.exp2(torch.floor(torch.log2(o.abs().clamp(min=1e-300))) - 7)
    dx = do @ p.w[name].abs().t() + _sum_slack(p, o, name)
    return final_bound(fw, bf16, dx)


# ---- 3. lm_head with integer operands -------------------------------------------------------------------------------------------------

def lm_head_probe(B, T, V, seed=0):
    """Every output projection zero: the final norm sees x0.  lm_head integers in [-3, 3], final_ln integers in [1, 4]: a bf16
    handle's logits are the integers `p.want` (every partial sum is below 512 * 12 < 2^24) bit for bit."""
    gen = torch.Generator().manual_seed(70001 * seed + 13 * V + B)
    p = _base(B, T, gen, V=V)
    p.w["lm_head"] = torch.randint(-3, 4, (V, D), generator=gen).double()
    p.w["final_ln"] = torch.randint(1, 5, (D,), generator=gen).double()
    p.want = (p.x0 * p.w["final_ln"]) @ p.w["lm_head"].t()
    assert D * 3 * 4 < ex.EXACT_F32
    return p


def lm_head_f32_bound(p, ref):
    """f32 handles, from the chain of dec_norm_gemv<float, 0>: rstd = rsqrtf(1 + eps) carries <= 3 u (the sum 1 + eps u / 2,
    halved by the root; rsqrtf <= 2 u), every term lw * (x * rstd) one rounding, and a logit is 8 fused multiply-adds and a
    6-level butterfly deep: 14 roundings of partial sums no larger than S = sum_k |lm[n][k]| final_ln[k]."""
    S = p.w["final_ln"] @ p.w["lm_head"].abs().t()
    return U * (3 * ref.abs() + 15 * S)


# ---- 4 / 5. residual projections and the gated GELU ---------------------------------------------------------------------------------

RMS_U = 26      # the final norm of a residual row in f32: 512 squares summed 32 + 5 deep (<= 40 u on the sum, 20 u on its root),
                # + eps and rsqrtf (3 u), lw * (x * rstd) (2 u)
SUM_U = 24      # a residual element: operands off by <= 8 u (an f32 handle's normed inputs), 8 fused multiply-adds, a 6-level
                # butterfly and the residual add, each one rounding of a partial sum <= S_x = |x0| + sum_j |W[n][j]| |a[j]|
                # (the matrix-core kernels serve bf16 handles only: their products are exact, and their sums are exact dyadic
                # numbers in probe 4 and three bf16 values in probe 5, far inside this)


def final_bound(fw, bf16, dx):
    """|logit - fw.v| for an identity lm_head and final_ln = 1, given `dx`, the absolute uncertainty of every element of the
    final residual: dx through the scale, RMS_U u of the value, the move of rstd when the row's elements move by dx, and for a
    bf16 handle one rounding of the normed value to bf16 (half an ulp, <= 2^-8 |v|)."""
    ss = (fw.x * fw.x).sum(-1, keepdim=True)
    rel = RMS_U * U + (fw.x.abs() * dx).sum(-1, keepdim=True) / ss + (2.0 ** -8 if bf16 else 0.0)
    return fw.rstd * dx + fw.v.abs() * rel


def _sum_slack(p, a, name):
    return SUM_U * U * (p.x0.abs() + a.abs() @ p.w[name].abs().t())


def _sparse_rows(n_rows, K, cover, gen):
    """[n_rows, K] in {-1, 0, 1}: every column k is covered by `cover` distinct rows."""
    w = torch.zeros(n_rows, K, dtype=F64)
    for k in range(K):
        w[torch.randperm(n_rows, generator=gen)[:cover], k] = _pm1((cover,), gen)
    return w


def res_inner_probe(B, T, Lc, seed=0):
    """Probe 2's cross-attention with w_o_cross sparse in {-1, 0, 1}, every k covered by 3 rows: the residual is an exact
    dyadic number (o is a multiple of 1/2) and the only inexact step left is the final norm."""
    for attempt in range(16):
        gen = torch.Generator().manual_seed(80021 * seed + 17 * Lc + B + 1000003 * attempt)
        p = cross_attention_probe(B, T, Lc, gen=gen)
        p.w["w_o_cross"] = _sparse_rows(D, INNER, 3, gen)
        p.x_want = p.x0 + p.o_want @ p.w["w_o_cross"].t()
        if float(p.x_want.abs().max()) <= X_MAX:
            return p
    raise AssertionError("no res_inner probe with |x| <= %d" % X_MAX)


def res_inner_bound(p, fw, bf16):
    return final_bound(fw, bf16, _sum_slack(p, fw.o_cross, "w_o_cross"))


def res_ff_probe(B, T, seed=0):
    """A known g: wi_0 rows select a dim where ln_ff = 6, so h0 = +-6 and gelu_new(h0) is 6 or 0 (tanhf has saturated: 1 - tanh
    < 2e-11); wi_1 rows select a dim where ln_ff = 1, h1 = +-1; g is 0 or +-6.  w_wo sparse in {-1, 0, 1}, 4 entries per row,
    every k covered by 2 rows: |x| <= 25."""
    for attempt in range(16):
        gen = torch.Generator().manual_seed(90011 * seed + B + 1000003 * attempt)
        p = _base(B, T, gen)
        dims = torch.randperm(D, generator=gen)
        big, one = dims[:D // 2], dims[D // 2:]
        p.w["ln_ff"][big] = 6
        n = torch.arange(DFF)
        p.w["w_wi"][n, big[torch.randint(0, D // 2, (DFF,), generator=gen)]] = _pm1((DFF,), gen)
        p.w["w_wi"][DFF + n, one[torch.randint(0, D // 2, (DFF,), generator=gen)]] = _pm1((DFF,), gen)
        r = torch.arange(D)
        shift = (r + 1 + int(torch.randint(0, D - 2, (1,), generator=gen))) % D
        for cols in (r, r + D, shift, shift + D):
            p.w["w_wo"][r, cols] = _pm1((D,), gen)
        xn = p.x0 * p.w["ln_ff"]
        h0, h1 = xn @ p.w["w_wi"][:DFF].t(), xn @ p.w["w_wi"][DFF:].t()
        p.g_want = torch.where(h0 > 0, h0, torch.zeros_like(h0)) * h1
        p.x_want = p.x0 + p.g_want @ p.w["w_wo"].t()
        if float(p.x_want.abs().max()) <= X_MAX:
            return p
    raise AssertionError("no res_ff probe with |x| <= %d" % X_MAX)


def geglu_probe(B, T, seed=0):
    """ln_ff = 1 and w_wi sparse in {-1, 0, 1} with 1..4 entries per row: h0, h1 are exact integers in [-4, 4].  w_wo selects
    two g per residual dim through a random permutation."""
    gen = torch.Generator().manual_seed(100019 * seed + B)
    p = _base(B, T, gen)
    nnz = torch.randint(1, 5, (2 * DFF,), generator=gen)
    for n in range(2 * DFF):
        c = torch.randperm(D, generator=gen)[:int(nnz[n])]
        p.w["w_wi"][n, c] = _pm1((len(c),), gen)
    sel = torch.randperm(DFF, generator=gen)
    r = torch.arange(D)
    p.w["w_wo"][r, sel[:D]] = 1
    p.w["w_wo"][r, sel[D:]] = 1
    return p


def g_uncertainty(fw, bf16):
    """(dg, wide): the absolute uncertainty of every g = gelu_new(h0) * h1 as the kernels compute it, against `fw.g`.
    The f32 chain: the argument of tanhf carries <= 6 u (relative), which moves tanh by <= 6 u * max(a sech^2 a) < 3 u; tanhf
    itself <= 5 ulp = 5 u below 1; 1 + tanh, 0.5 x (.) and the product with h1 one rounding each: d32 = 5 u |h0 h1| + 2 u |g|.
    An f32 handle's h0, h1 are themselves off by <= 8 u relative (gelu' <= 1.13): + 9 u |h0 h1| + 8 u |g|.
    A bf16 handle rounds g to bf16 (ulp = one bf16 ulp of g):
      * d32 >= ulp / 4 (the deep negative tail, where 1 + tanh cancels): two roundings of values d32 apart differ by at
        most d32 + ulp <= 5 d32, an f32-sized error: dg = d32 + ulp;
      * else, no bf16 tie within max(d32, TIE_REL |g|) of the exact g: the kernel rounds to the very bf16 the reference
        holds, dg = 0;
      * else (`wide`, the elements WIDE_CAP counts): dg = d32 + ulp."""
    g = gelu_new(fw.h0) * fw.h1
    hh = (fw.h0 * fw.h1).abs()
    if not bf16:
        return U * (14 * hh + 10 * g.abs()), torch.zeros_like(g, dtype=torch.bool)
    d32 = U * (5 * hh + 2 * g.abs())
    a = g.abs().clamp(min=1e-300)
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    frac = a / ulp - torch.floor(a / ulp)
    tail = d32 >= ulp / 4
    wide = ~tail & ((frac - 0.5).abs() * ulp <= torch.maximum(d32, TIE_REL * a))
    return torch.where(tail | wide, d32 + ulp, torch.zeros_like(g)), wide


def ffn_bound(p, fw, bf16):
    """Probes 4 (res_ff) and 5: (bound [B, T, 512], share of the logits that got the widened bound)."""
    dg, wide = g_uncertainty(fw, bf16)
    absw = p.w["w_wo"].abs().t()
    dx = dg @ absw + _sum_slack(p, fw.g, "w_wo")
    return final_bound(fw, bf16, dx), float(((wide.double() @ absw) > 0).double().mean())


# ---- one entry for the CPU proof and the device tests -------------------------------------------------------------------------------

def reference(p, bf16):
    """`forward` in float64, computed once per probe and handle type (shared, never modified)."""
    cache = p.__dict__.setdefault("_fw", {})
    if bf16 not in cache:
        cache[bf16] = forward(p, bf16)
    return cache[bf16]


def check(kind, p, logits, bf16, what):
    """The probe's assertion on logits [B, T, V] of a bf16 or f32 handle; returns the largest error / bound (the figure a
    `RATIO` line prints; 0 for the bit-exact case)."""
    if kind in ("self", "cross"):
        return check_attention(p, logits, what)
    if kind == "lm_head":
        if bf16:
            check_equal(what, logits, p.want.float())
            return 0.0
        ref = reference(p, False).logits
        return check_within(what, logits, ref, lm_head_f32_bound(p, ref))
    fw = reference(p, bf16)
    if kind == "res_inner":
        return check_within(what, logits, fw.v, res_inner_bound(p, fw, bf16))
    if kind in ("q_cross", "q_self"):
        return check_within(what, logits, fw.v, soft_bound(p, fw, bf16, kind[2:]))
    assert kind in ("res_ff", "geglu"), kind
    bound, share = ffn_bound(p, fw, bf16)
    assert share <= WIDE_CAP, (what, share)
    return check_within(what, logits, fw.v, bound)
