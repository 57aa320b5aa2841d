"""Constructions and host rules of the element-exact tests of the decode tail (csrc/decode_tail.hip): tail probes.
Proven on the CPU by tests/test_exact_tail_cpu.py, run on the device by tests/test_exact_tail_gpu.py.  Plain torch and numpy;
nothing here touches the library.

A tail probe is a one-layer decoder (tests/_exact_decode.py `_base`: every sublayer projection zero) that runs TOKEN steps.  The
512 dimensions are four blocks:

  token    [0, 64)     embed[token] is the +-1 code of class(token) = token % 64 (+1 at the class, -1 elsewhere); pos is 0
  position [64, 128)   pos[p] is the +-1 code of p; embed is 0
  row      [128, 384)  0 in embed and pos; the cross-attention (enc_len = 1, w_q_cross = 0: the softmax over one key is exactly
                       1) adds cross V of row b, the +-1 code of b, through a 0/1 selection w_o_cross
  constant [384, 512)  pos is +1, embed is 0

so the residual that reaches the final norm is +-1 at all 512 elements (rstd = 1 after the bf16 rounding, final_ln = 1).  With
integer tables WE [V, 64], WP [V, T], WR [V, B] in the three coded blocks of lm_head and their row sums spread over the constant
block, the logits of row b at step t after token `tok` are the integers

      logit[b, t, n] = 2 * (WE[n, tok % 64] + WP[n, t] + WR[n, b])

bit for bit on a bf16 handle.  An lm_head entry of +inf at position dimension s makes a column -inf at every step but s, where it
is +inf; +inf at s and at a spare dimension makes it NaN at step s.  The host therefore knows every step's logits of every row
and derives the whole decode by the documented rule: `GreedyRef` (torch.argmax, float64 log_softmax, tests/sample_ref.py for a
drawn token), `BeamRef` of tests/beam_ref.py.  On an f32 handle the logits are within `_exact_decode.lm_head_f32_bound` of the
design, the rule is applied to the copied logits, and only columns with identical lm_head rows (`identical_columns`) are designed ties.
The reorder probes at the end of the file are two-layer decoders of their own; their section says how they are built."""
from types import SimpleNamespace

import numpy as np
import torch

import _exact_decode as ed
import sample_ref as sr
from beam_ref import BeamRef

D, INNER = ed.D, ed.INNER
TOK0, NTOK = 0, 64
POS0, NPOS = 64, 64
ROW0, NROW = 128, 256
CON0, NCON = 384, 128
SPARE_POS = NPOS - 1                    # a position no run reaches: its dimension is -1 at every step
START, EOS, PAD = 0, 1, 0
STEPS = 16                              # token steps of the greedy and sampled probes
LOGP_TOL = 2e-5                         # tests/test_sample_gpu.py
F64 = torch.float64
NEG = float("-inf")


# ---- the probe ---------------------------------------------------------------------------------------------------------------------

def _code(idx, n):
    """[len(idx), n] +-1: +1 at idx, -1 elsewhere."""
    c = -np.ones((len(idx), n))
    c[np.arange(len(idx)), idx] = 1
    return c


def _spread(S):
    """[V] integers -> [V, NCON] integers of magnitude <= 128 with those row sums."""
    out, rem = np.zeros((len(S), NCON)), S.astype(np.float64).copy()
    for j in range(NCON):
        out[:, j] = np.clip(rem, -128, 128)
        rem -= out[:, j]
    assert not rem.any(), "row sums too large for the constant block"
    return out


def tail_probe(B, T, V, WE, WP, WR, infs=()):
    """The probe of the tables WE [V, 64], WP [V, T], WR [V, B] (integers); infs: (column, position s) puts +inf at position
    dimension s of that lm_head row.  `p.w`, `p.ck`, `p.cv` as `_exact_decode._base`; `p.embed` [V, 512], `p.pos` [T + 2, 512]."""
    assert T < SPARE_POS and B <= NROW and WE.shape == (V, NTOK) and WP.shape == (V, T) and WR.shape == (V, B)
    p = ed._base(B, T, torch.Generator().manual_seed(0), V=V)
    del p.x0
    lm = np.zeros((V, D))
    lm[:, TOK0:TOK0 + NTOK] = WE
    lm[:, POS0:POS0 + T] = WP
    lm[:, ROW0:ROW0 + B] = WR
    lm[:, CON0:] = _spread(WE.sum(1) + WP.sum(1) + WR.sum(1))
    for col, s in infs:
        lm[col, POS0 + s] = np.inf
    p.w["lm_head"] = torch.from_numpy(lm)
    p.w["w_o_cross"][ROW0 + torch.arange(NROW), torch.arange(NROW)] = 1
    p.cv[:, 0, :NROW] = torch.from_numpy(_code(np.arange(B), NROW))
    embed = np.zeros((V, D))
    embed[:, TOK0:TOK0 + NTOK] = _code(np.arange(V) % NTOK, NTOK)
    pos = np.zeros((T + 2, D))
    pos[:, POS0:POS0 + NPOS] = _code(np.arange(T + 2), NPOS)
    pos[:, CON0:] = 1
    p.embed, p.pos = torch.from_numpy(embed), torch.from_numpy(pos)
    p.WE, p.WP, p.WR, p.infs = WE, WP, WR, tuple(infs)
    return p


def residual(p, tok, t):
    """The residual the final norm sees at step t after tokens `tok` [B]: embed[tok] + pos[t] + the injected row code."""
    x = p.embed[torch.as_tensor(tok)] + p.pos[t]
    x[:, ROW0:ROW0 + NROW] += p.cv[:, 0, :NROW]
    return x


def design_logits(p, tok, t):
    """[B, V] float64: lm_head x residual, the infinite entries of lm_head taken separately (+inf and -inf terms give NaN)."""
    x = residual(p, tok, t)
    if "_lm" not in p.__dict__:
        lm = p.w["lm_head"]
        fin = torch.isfinite(lm)
        sign = torch.where(fin, torch.zeros_like(lm), torch.sign(lm))
        p._lm = (torch.where(fin, lm, torch.zeros_like(lm)).t().contiguous(), sign.clamp(min=0).t().contiguous(),
                 (-sign).clamp(min=0).t().contiguous())
    lmf, sp, sn = p._lm
    out = x @ lmf
    xp, xn = x.clamp(min=0), (-x).clamp(min=0)
    up = (xp @ sp + xn @ sn) > 0
    down = (xp @ sn + xn @ sp) > 0
    out = torch.where(up, torch.full_like(out, float("inf")), out)
    out = torch.where(down, torch.full_like(out, NEG), out)
    return torch.where(up & down, torch.full_like(out, float("nan")), out)


def check_tail_probe(p, tokens=None):
    """The construction conditions: operands a bf16 holds, a +-1 residual at every step, partial sums below 2^24, the closed
    form of the finite logits."""
    for name, t in list(p.w.items()) + [("ck", p.ck), ("cv", p.cv), ("embed", p.embed), ("pos", p.pos)]:
        assert torch.equal(ed._bf16(t), t), name
    lm = p.w["lm_head"]
    assert float(torch.where(torch.isfinite(lm), lm, torch.zeros_like(lm)).abs().sum(1).max()) < 2.0 ** 24
    assert p.Lc == 1 and not p.w["w_q_cross"].any() and not p.ck.any()      # one key, score 0: the softmax is exactly 1
    for name in ("w_qkv", "w_o_self", "w_wi", "w_wo"):
        assert not p.w[name].any(), name
    rows = torch.arange(p.B)
    for t in range(p.T + 1):
        tok = (rows * 7 + t * 3) % p.V if tokens is None else tokens[:, t]
        x = residual(p, tok, t)
        assert bool((x.abs() == 1).all()), t
        if t < p.T:
            want = 2.0 * (p.WE[:, np.asarray(tok) % NTOK].T + p.WP[:, t][None, :] + p.WR.T)
            lg = design_logits(p, tok, t)
            ok = torch.isfinite(lg)
            assert torch.equal(lg[ok], torch.from_numpy(want)[ok]), t
            cols = sorted({c for c, _ in p.infs})
            assert bool(ok[:, [c for c in range(p.V) if c not in cols]].all())


# ---- comparisons that take NaN as NaN -----------------------------------------------------------------------------------------------

def check_equal(what, got, want):
    """`_exact_decode.check_equal`, a NaN equal to a NaN."""
    g, w = torch.as_tensor(got), torch.as_tensor(want).to(torch.as_tensor(got).dtype)
    if g.is_floating_point():
        ed.check_equal(what + " (NaN mask)", torch.isnan(g).to(torch.int8), torch.isnan(w).to(torch.int8))
        g, w = torch.nan_to_num(g, nan=0.0, posinf=float("inf"), neginf=NEG), torch.nan_to_num(w, nan=0.0, posinf=float("inf"),
                                                                                              neginf=NEG)
    ed.check_equal(what, g, w)


def check_within(what, got, ref, bound):
    """`_exact_decode.check_within` on the elements finite in `ref`; the others (NaN, +-inf) must be the same in `got`."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    odd = ~torch.isfinite(ref)
    cls = lambda t: torch.where(torch.isnan(t), torch.full_like(t, 3.0), torch.sign(t) * (~torch.isfinite(t)).double())
    ed.check_equal(what + " (NaN / inf)", cls(got), cls(ref))
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref)
    z = torch.zeros_like(ref)
    return ed.check_within(what, torch.where(odd, z, got), torch.where(odd, z, ref), torch.where(odd, z + 1, bound))


def f32_bound(p, ref):
    """`_exact_decode.lm_head_f32_bound` with the infinite lm_head entries left out of S (their columns are never finite)."""
    lm = p.w["lm_head"]
    q = SimpleNamespace(w=dict(final_ln=p.w["final_ln"], lm_head=torch.where(torch.isfinite(lm), lm, torch.zeros_like(lm))))
    ref = torch.as_tensor(ref).double()
    return ed.lm_head_f32_bound(q, torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref)))


# ---- the greedy and the sampled rule ----------------------------------------------------------------------------------------------------
# Faults (the emulation of the CPU proof only): "tie_high" (the highest index of equal maxima), "nan_loses", "nan_second",
# "ban_after" (the ban is applied to the numbers only: a banned NaN still wins), "col_v" (the element after the row takes part
# as column V), "no_pad" (a finished row goes on emitting its argmax), "pad_logp" (a pad carries the argmax's log-probability),
# "fin_late" (ST_FIN one step on), "row_next" (row b draws with row b + 1's counter), "step_next" (step t + 1's).

def _argmax(m, fault):
    if fault == "nan_loses":
        return torch.argmax(torch.nan_to_num(m, nan=NEG), -1)
    if fault == "nan_second":
        nan = torch.isnan(m)
        second = nan & (nan.cumsum(-1) == 2)
        return torch.where(second.any(-1), second.int().argmax(-1), torch.argmax(m, -1))
    if fault == "tie_high":
        return m.shape[-1] - 1 - torch.argmax(m.flip(-1), -1)
    return torch.argmax(m, -1)


class GreedyRef:
    """The greedy / sampled tail and the state block, step by step on given logits.  ban: [V] bool or None; sampling: None or
    (seed, temperature, top_k, top_p)."""

    def __init__(self, B, V, ban=None, sampling=None, fault=None):
        self.B, self.V, self.ban, self.sampling, self.fault = B, V, None if ban is None else torch.as_tensor(ban, dtype=torch.bool), \
            sampling, fault
        self.done = torch.zeros(B, dtype=torch.bool)
        self.t, self.all, self.fin = 0, 0, -1
        self.edge = []                              # per step: distance of every drawing row's u to an interval edge

    def masked(self, lg):
        m = lg.float().clone()
        if self.ban is not None:
            if self.fault == "ban_after":
                m[:, self.ban] = torch.where(torch.isnan(m[:, self.ban]), m[:, self.ban], torch.full_like(m[:, self.ban], NEG))
            else:
                m[:, self.ban] = NEG
        return m

    def step(self, lg):
        """lg [B, V]: this step's logits.  -> (tokens [B] int64, log-probabilities [B] float64, poll triple)."""
        m = self.masked(lg)
        if self.fault == "col_v":                   # what lies after row b: row b + 1's column 0 (nothing after the last row)
            m = torch.cat([m, torch.cat([lg.float()[1:, :1], torch.full((1, 1), NEG)])], 1)
        tok = _argmax(m, self.fault)
        if self.sampling is not None:
            seed, temp, top_k, top_p = self.sampling
            rows = sr.sample_ref(m.numpy(), None, temp, top_k, top_p)
            r, s = np.arange(self.B), self.t
            if self.fault == "row_next":
                r = r + 1
            if self.fault == "step_next":
                s = s + 1
            u = sr.uniform(seed, r, s)
            tok = torch.from_numpy(rows.pick(u)).long()
            self.edge.append(np.where(self.done.numpy(), np.inf, rows.edge_distance(u)))
        lsm = torch.log_softmax(m.double(), -1)
        lp = lsm.gather(1, tok[:, None])[:, 0]
        was = self.done.clone()
        if self.fault != "no_pad":
            tok = torch.where(was, torch.full_like(tok, PAD), tok)
        if self.fault != "pad_logp":
            lp = torch.where(was, torch.zeros_like(lp), lp)
        self.done = was | (tok == EOS)
        if bool(self.done.all()) and not self.all:
            self.all, self.fin = 1, self.t + (1 if self.fault == "fin_late" else 0)
        self.t += 1
        return tok, lp, (self.t, self.all, self.fin)


def greedy_trace(p, ban=None, sampling=None, fault=None, copy=None, T=None):
    """The decode of probe p by the rule.  `copy` [B, T, V]: apply the rule to these logits (an f32 handle's copy) instead of
    the design.  -> tokens [B, T], logp [B, T] f64, polls [T, 3], logits [B, T, V] f64 (the DESIGN along the emitted tokens),
    active [B, T] (the row had not finished before the step), edge [B, T]."""
    T = T or p.T
    ref = GreedyRef(p.B, p.V, ban, sampling, fault)
    tok = torch.full((p.B,), START, dtype=torch.long)
    toks, lps, polls, lgs, act = [], [], [], [], []
    for t in range(T):
        lg = design_logits(p, tok.clamp(max=p.V - 1), t)
        act.append(~ref.done.clone())
        tok, lp, poll = ref.step(lg if copy is None else copy[:, t])
        toks.append(tok), lps.append(lp), polls.append(poll), lgs.append(lg)
    r = SimpleNamespace(tokens=torch.stack(toks, 1), logp=torch.stack(lps, 1), polls=torch.tensor(polls), logits=torch.stack(lgs, 1),
                        active=torch.stack(act, 1))
    r.edge = np.stack(ref.edge, 1) if ref.edge else None
    return r


def check_greedy(what, got, ref, logp=True):
    """The device's (or a faulty emulation's) tokens [B, T], logp [B, T] and polls [T, 3] against the rule's, per (row, step)."""
    ed.check_equal(what + " tokens", got.tokens[..., None], ref.tokens[..., None])
    ed.check_equal(what + " poll (step, field, -)", got.polls[..., None, None].int(), ref.polls[..., None, None].int())
    if not logp:
        return 0.0
    pads = ~ref.active
    assert bool((got.logp[pads] == 0).all()), what + ": the log-probability of a pad is not 0.0"
    return check_within(what + " logp", got.logp[..., None], ref.logp[..., None], LOGP_TOL)


# ---- the greedy designs -------------------------------------------------------------------------------------------------------------------

WIN, LOW = 3, -4                                    # a scene's winners hold logit 2 * WIN; a featured column off scene 2 * LOW
NAN1, NAN2, NAN3, NAN4, PINF = 17, 30, 23, 31, 35   # NaN at steps 11 + 12, 12, 13, 12; +inf at step 14 (-inf at every other step)
FIN_OPEN = (7.5, 12, 3, 15, 0.5, 9, 5, 14, 10, 2, 6)      # x.5: a tie with the scene's winner at step x instead of a win
FIN_CLOSED = (0.5, 4, 9, 2, 8, 7.5, 5, 6)


def _scenes(V):
    """step -> [(column, level)]: what the position table puts on top at each step."""
    uniq = []
    for c in (0, 63, 64, 511, 512, V - 1):
        if c < V and c not in uniq:
            uniq.append(c)
    sc = {t: [(c, WIN)] for t, c in enumerate(uniq)}
    lane = (5, 69) if V > 69 else (0, 64) if V > 64 else (2,)
    sc[6] = [(c, WIN) for c in lane]                                          # one lane, different i
    sc[7] = [(7, WIN), (8, WIN)]                                              # neighbouring lanes
    sc[8] = [(c, WIN) for c in (3, 10, 75, 140, 600, 1100, V - 1) if c < V]   # many members, the last column among them
    sc[9] = [(c, WIN) for c in (9, 521, 1033) if c < V]                       # one lane and slot, different 512-column passes
    sc[10] = [(c, WIN) for c in (12, 13, 78) if c < V]                        # 12 is banned
    sc[15] = [(20, WIN + 3), (21, WIN)]                                       # 20 is banned: the runner-up wins
    for t in range(STEPS):
        sc.setdefault(t, [(2, WIN)])
    return sc


def greedy_ban(V):
    ban = np.zeros(V, dtype=bool)
    ban[[12, 20, NAN1]] = True
    ban[np.arange(36, V, 3)] = True
    feat = {c for s in _scenes(V).values() for c, _ in s} - {12, 20}
    ban[sorted(feat)] = False
    ban[EOS] = False
    return ban


def greedy_design(V, B, variant):
    """variant "open": the last row never emits EOS; "closed": every row has by step 10; "inf" (V = 40): every column is
    +-inf at every step (column n is +inf at step n % 8, EOS never) and the steps from 8 on are rows of -inf alone."""
    T = STEPS
    rng = np.random.default_rng([V, B, len(variant)])
    if variant == "inf":
        z = np.zeros((V, T), dtype=np.int64)
        infs = [(n, n % 8 if n != EOS else SPARE_POS) for n in range(V)]
        return tail_probe(B, T, V, np.zeros((V, NTOK), dtype=np.int64), z, np.zeros((V, B), dtype=np.int64), infs)
    sc = _scenes(V)
    feat = sorted({c for s in sc.values() for c, _ in s} | {EOS, NAN1, NAN2, NAN3, NAN4, PINF})
    WE, WR, WP = rng.integers(0, 2, (V, NTOK)), rng.integers(-2, 1, (V, B)), np.full((V, T), -1)
    WE[feat], WR[feat], WP[feat] = 0, 0, LOW
    WR[0] = np.arange(B) % 2                        # column 0 of an odd row is one step higher: it beats the row before's maximum
    for t, s in sc.items():
        for c, lv in s:
            WP[c, t] = lv
    fins = FIN_OPEN if variant == "open" else FIN_CLOSED
    f = np.array([fins[(b + b // 8) % len(fins)] for b in range(B)])
    WP[EOS] = 2 * np.arange(T)                      # EOS of row b at step t: 2 t + WR[EOS, b]
    WR[EOS] = np.where(f % 1 > 0, WIN - 2 * np.floor(f), WIN + 1 - 2 * f)      # a tie with the winners at step x, or a win at f
    if variant == "open":
        WR[EOS, B - 1] = -60
    infs = [(NAN1, 11), (NAN1, 12), (NAN2, 12), (NAN2, SPARE_POS), (NAN3, 13), (NAN3, SPARE_POS), (NAN4, 12), (NAN4, SPARE_POS),
            (PINF, 14)]
    return tail_probe(B, T, V, WE, WP, WR, infs)


def identical_columns(p):
    """Groups of columns whose lm_head rows are the same: their logits are equal bits on any handle (equal operands in equal
    order), the ties an f32 handle keeps."""
    groups = {}
    for c, row in enumerate(p.w["lm_head"].numpy()):
        groups.setdefault(row.tobytes(), []).append(c)
    return [g for g in groups.values() if len(g) > 1]


# ---- the scenario ledger of a greedy trace -----------------------------------------------------------------------------------------------

def greedy_ledger(p, tr, ban=None):
    """The scenarios the rows of trace `tr` meet while they are active (on the design's logits)."""
    V, out = p.V, set()
    ban = np.zeros(V, dtype=bool) if ban is None else np.asarray(ban, dtype=bool)
    fin_step = {}
    for b in range(p.B):
        for t in range(tr.tokens.shape[1]):
            if not bool(tr.active[b, t]):
                continue
            raw = tr.logits[b, t].numpy()
            m = np.where(ban, NEG, raw)
            tok = int(tr.tokens[b, t])
            if tok == EOS:
                fin_step[b] = t
            if np.isnan(raw[ban]).any() and not np.isnan(m).any():
                out.add("nan:banned")
            if np.isnan(m).any():
                out.add("nan:1" if np.isnan(m).sum() == 1 else "nan:2")
                if np.isnan(raw[ban]).any() and np.flatnonzero(np.isnan(raw))[0] < np.flatnonzero(np.isnan(m))[0]:
                    out.add("nan:first-banned")
                continue
            if (raw == NEG).all():
                out.add("all-neginf")
                continue
            if ban.all():
                out.add("all-banned")
                continue
            top = m.max()
            if top == np.inf and np.isfinite(m).any():
                out.add("inf:finite")
            M = np.flatnonzero(m == top)
            rawM = np.flatnonzero(raw == np.nanmax(raw))
            if len(rawM) == 1 and ban[rawM[0]]:
                out.add("max-banned")
            rawT = np.flatnonzero(raw == top)
            if len(rawT) > len(M) and rawT[0] < M[0]:
                out.add("tie:lowest-banned")
            if len(M) == 1:
                for name, c in (("0", 0), ("63", 63), ("64", 64), ("511", 511), ("512", 512), ("last", V - 1)):
                    if M[0] == c:
                        out.add("max@" + name)
                continue
            assert tok == M[0]
            out.add("tie:many" if len(M) > 2 else "tie:two")
            lanes, slots, passes = M % 64, (M % 512) // 64, M // 512
            pairs = [(i, j) for i in range(len(M)) for j in range(i + 1, len(M))]
            if any(lanes[i] == lanes[j] and passes[i] == passes[j] for i, j in pairs):
                out.add("tie:lane")
            if any(lanes[i] != lanes[j] for i, j in pairs):
                out.add("tie:lanes")
            if any(passes[i] != passes[j] and lanes[i] == lanes[j] and slots[i] == slots[j] for i, j in pairs):
                out.add("tie:passes")
            if M[-1] == V - 1:
                out.add("tie:last")
            if EOS in M:
                out.add("eos:tie-higher" if M[0] == EOS else "eos:tie-lower")
    steps = tr.tokens.shape[1]
    pairs = [(a, b) for a in fin_step for b in fin_step if a < b and fin_step[a] != fin_step[b]]
    if any(a // 8 == b // 8 for a, b in pairs):
        out.add("fin:same-wg")
    if any(a // 8 != b // 8 for a, b in pairs):
        out.add("fin:diff-wg")
    if len(fin_step) == p.B:
        out.add("fin:all")
        if max(fin_step.values()) < steps - 1:
            out.add("fin:early")
        assert int(tr.polls[-1, 1]) == 1 and int(tr.polls[-1, 2]) == max(fin_step.values())
    else:
        out.add("fin:never")
        assert int(tr.polls[-1, 1]) == 0 and int(tr.polls[-1, 2]) == -1
    return out


def greedy_required(V, B, banned):
    """What the open and the closed probe of (V, B) must reach between them, without and with the ban."""
    need = {"max@0", "max@last", "tie:two", "tie:many", "tie:lanes", "tie:last", "nan:1", "nan:2", "inf:finite", "eos:tie-higher",
            "eos:tie-lower", "fin:never", "fin:all", "fin:early", "fin:same-wg"}
    need |= {"max@63"} if V > 64 else set()
    need |= {"max@64", "tie:lane"} if V > 64 else set()
    need |= {"max@511", "max@512", "tie:passes"} if V > 1033 else ({"max@511"} if V == 512 else set())
    if banned:
        need |= {"tie:lowest-banned", "nan:banned", "nan:first-banned", "max-banned"}
    if B > 8:
        need |= {"fin:diff-wg"}
    return need


# ---- the sampled cases ---------------------------------------------------------------------------------------------------------------------
# (id, V, rows, bf16, banned, top_k, two seeds) on the open probe, temperature 1 and top_p 1.  The seeds were searched on the host
# rule alone so that no draw lies within 2 SLACK of an interval edge (tests/test_exact_tail_cpu.py asserts SLACK): the device
# must then return the host's token for every (row, step).  The nine-row cases at 1536 columns set top_k = 40 (78 draws among
# 1536 edges leave no such seed); an f32 handle's near-ties would split the groups of equal logits that top_k keeps whole, so
# its cases keep every column.
SAMPLED = [
    ("bf16-b9-v1536", 1536, 9, True, False, 40, (3, 4)),
    ("bf16-b9-v1536-ban", 1536, 9, True, True, 40, (3, 5)),
    ("f32-b3-v1536", 1536, 3, False, False, 0, (2, 19)),
    ("f32-b3-v1536-ban", 1536, 3, False, True, 0, (3, 7)),
    ("bf16-b9-v40", 40, 9, True, False, 0, (1, 2)),
    ("bf16-b9-v40-ban", 40, 9, True, True, 0, (1, 2)),
    ("f32-b3-v40", 40, 3, False, False, 0, (1, 2)),
    ("f32-b3-v40-ban", 40, 3, False, True, 0, (1, 2)),
]


# ---- beam search: the designs -----------------------------------------------------------------------------------------------------------
# Live columns hold logits near the top, every other column 2 * DEAD.  Tokens whose classes share class // 2 have the same WE
# column, so two beams that took such twins at equal scores go on with identical logit rows (in groups whose WR depends on the
# group alone): the three designed tie classes are (1) equal logits within a row, (2) identical rows under equal beam scores,
# (3) -inf candidates.

DEAD = -15


def beam_live(V, k):
    big = [c for c in (68, 69, 516, 517, 1100, 1101, V - 2, V - 1) if 40 < c < V]
    small = list(range(4, 16)) + ([38, 39] if V == 40 else [])
    return sorted(set([0, EOS] + small + big + (list(range(20, 28)) if k > 4 else [])))


def beam_design(V, k, G, T, seed, nan_last=False):
    """The bf16 handles' design, random over the live columns: WP in 0..3 with twins (columns 2 m, 2 m + 1) mostly equal, WE by
    class // 2, WR by group % 4 (odd groups add a term per beam, so their rows are never identical), EOS shifted per group."""
    rng = np.random.default_rng([V, k, G, T, seed])
    B, live = G * k, np.array(beam_live(V, k))
    WE, WP, WR = np.zeros((V, NTOK), dtype=np.int64), np.full((V, T), DEAD), np.zeros((V, B), dtype=np.int64)
    WE[live] = np.repeat(rng.integers(0, 2, (len(live), NTOK // 2)), 2, 1)
    wp = rng.integers(0, 4, (len(live), T))
    twin = {c: i for i, c in enumerate(live)}
    for i, c in enumerate(live):
        if c % 2 and c - 1 in twin and c != EOS:
            same = rng.random(T) < 0.7
            wp[i] = np.where(same, wp[twin[c - 1]], wp[i])
    WP[live] = wp
    WP[EOS] = rng.integers(-1, 4, T)
    g, j = np.arange(B) // k, np.arange(B) % k
    WR[live] = rng.integers(0, 2, (len(live), 4))[:, g % 4] + (g % 2) * rng.integers(0, 2, (len(live), 8))[:, j]
    WR[EOS] += rng.integers(-2, 2, 4)[g % 4]
    # nan_last: live column 10 is NaN at the last step (and -inf before it): every row's log-softmax is NaN there
    p = tail_probe(B, T, V, WE, WP, WR, [(10, T - 1), (10, SPARE_POS)] if nan_last else ())
    p.k, p.G, p.live = k, G, live
    return p


def beam_design_f32(V, k, G, T, seed):
    """The f32 handles' design: only the ties an f32 handle keeps bit for bit.  Sums over different +-1 codes round differently in
    f32 even where they are equal in value, so equal bits need the same residual AND the same lm_head row.  Twins are duplicate
    lm_head rows (columns c, c + 64 where V allows: one class, so two beams that took them go on with the SAME residual and
    identical rows; c, c + 1 at V = 40, where only one beam runs); every other pair of live columns differs by >= 1 at every step
    (levels 3 x a permutation + WE in {0, 1}, EOS at 3 r + 2); WR is zero.  `BeamEmu(strict=p)` holds a design to that."""
    rng = np.random.default_rng([V, k, G, T, seed, 32])
    B = G * k
    base = list(range(4, 16)) + (list(range(20, 28)) if k > 4 else [])
    far = V > 128
    live = np.array(sorted([0, EOS] + base + ([c + 64 for c in base] if far else [])))
    pair = (lambda c: c % 64) if far else (lambda c: c // 2)
    pairs = sorted({pair(c) for c in live if c != EOS})
    level = np.stack([rng.permutation(len(pairs)) for _ in range(T)], 1)              # [pairs, T]: no two pairs alike at a step
    we = rng.integers(0, 2, (len(pairs), NTOK))
    WE, WP, WR = np.zeros((V, NTOK), dtype=np.int64), np.full((V, T), DEAD), np.zeros((V, B), dtype=np.int64)
    for c in live:
        if c != EOS:
            WE[c], WP[c] = we[pairs.index(pair(c))], 3 * level[pairs.index(pair(c))]
    WP[EOS] = 3 * rng.integers(0, len(pairs), T) + 2                                  # and EOS like none of them
    p = tail_probe(B, T, V, WE, WP, WR)
    p.k, p.G, p.live = k, G, live
    return p


def beam_ban(p, kind):
    """"some": a third of the live columns and of the dead ones; "eos-only": every token but EOS."""
    ban = np.zeros(p.V, dtype=bool)
    if kind == "eos-only":
        ban[:] = True
        ban[EOS] = False
    else:
        ban[np.arange(2, p.V, 3)] = True
        ban[EOS] = False
    return ban


def beam_tol(s):
    """`_tol` of tests/test_beam_decode_gpu.py: fp32 beam-score accuracy."""
    return 1e-5 + 4e-6 * np.abs(s)


class BeamEmu(BeamRef):
    """tests/beam_ref.py's search with a scenario ledger (`events`), the gaps behind every decision (`gaps`: kind, value,
    designed tie) and, for the CPU proof, one fault: "rank_desc" (equal candidates by flat index descending), "eos_low" (an EOS
    of rank >= k admitted), "drop_latest" (the latest of equal lowest hypotheses leaves), "best_first" (the first of equal best
    chosen), "done_gt" (is_done with > for >=).
    A score is equal BY DESIGN to another when both come from equal operands in equal order: `sid` names a beam score's
    lineage (the parent's lineage, the parent's whole logit row, the token's logit), so equal sid means equal bits on any
    device.  A zero gap between scores of different lineage is an accident of float64, and not allowed."""

    def __init__(self, *a, fault=None, strict=None, **kw):
        super().__init__(*a, **kw)
        self.fault, self.events, self.gaps = fault, set(), []
        # strict = the probe (f32 handles): a tie is designed only between candidates computed from the same residual (the
        # same class of token before, no row term) and duplicate lm_head rows, whatever the design's integers say
        self.strict = strict
        if strict is not None:
            assert not strict.WR.any()
            self.colid = [hash(row.tobytes()) for row in strict.w["lm_head"].numpy()]
            self.prev = [self.start] * (self.G * self.k)
        self.sid = [0 if r % self.k == 0 else 1 for r in range(self.G * self.k)]
        self.hsid = [[] for _ in range(self.G)]

    def _zero(self, kind, designed):
        self.gaps.append((kind, 0.0, bool(designed)))

    def _add(self, g, score, end, row, sid=None):
        h, hs = self.hyps[g], self.hsid[g]
        lowest = [i for i, e in enumerate(h) if e[0] == self.worst[g]]
        if len(h) >= self.k and score == score:
            if score == self.worst[g]:
                self._zero("admit", any(hs[i] == sid for i in lowest))
            else:
                self.gaps.append(("admit", abs(score - self.worst[g]), False))
        if len(h) < self.k or score > self.worst[g]:
            h.append((score, end, row))
            hs.append(sid)
            if len(h) > self.k:
                srt = sorted([(s, i) for i, (s, _, _) in enumerate(h)])
                drop = srt[0][1]
                if srt[0][0] == srt[1][0]:
                    self._zero("lowest", hs[srt[0][1]] == hs[srt[1][1]])
                    self.events.add("hyp:overflow-equal-lowest")
                    if self.fault == "drop_latest":
                        drop = [i for s, i in srt if s == srt[0][0]][-1]
                else:
                    self.gaps.append(("lowest", srt[1][0] - srt[0][0], False))
                self.events.add("hyp:overflow")
                del h[drop], hs[drop]
                self.worst[g] = srt[1][0]
            else:
                self.worst[g] = min(score, self.worst[g])

    def step(self, t, logits):
        G, k, V, ev = self.G, self.k, self.V, self.events
        x = np.asarray(logits, dtype=np.float64).reshape(G * k, V)
        with np.errstate(invalid="ignore"):
            m = x.max(-1, keepdims=True)
            logp = (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))
        if self.ban is not None:
            logp[:, self.ban] = -np.inf
        with np.errstate(invalid="ignore"):
            s = logp + self.scores[:, None]
        if self.strict is not None:
            cand = lambda r, tok: hash((self.sid[r], self.prev[r] % NTOK, self.colid[tok], t))
        else:
            rowid = [hash(x[r].tobytes()) for r in range(G * k)]
            cand = lambda r, tok: hash((self.sid[r], rowid[r], float(x[r, tok]), t))
        parents, tokens, new = np.arange(G * k), np.full(G * k, self.pad, dtype=np.int64), np.zeros(G * k)
        sid = [2] * (G * k)
        cur_len = t + 1
        if any(self.done) and not all(self.done):
            ev.add("group:done-while-others-run")
        for g in range(G):
            if self.done[g]:
                continue
            flat = s[g * k:(g + 1) * k].reshape(-1)
            idx = np.arange(flat.size)
            order = np.lexsort((-idx if self.fault == "rank_desc" else idx, -flat, ~np.isnan(flat)))[:2 * k + 1]
            top = flat[order]
            if np.isnan(top).any():
                ev.add("nan:row")
            if (flat != -np.inf).sum() < 2 * k:
                ev.add("ban:fewer-than-2k-live")
            for r in range(min(2 * k, len(order) - 1)):          # every gap that decides a rank
                (ja, ta), (jb, tb) = divmod(int(order[r]), V), divmod(int(order[r + 1]), V)
                ra, rb = g * k + ja, g * k + jb
                if np.isnan(top[r]) or np.isnan(top[r + 1]):
                    continue
                if top[r] != top[r + 1]:
                    self.gaps.append(("rank", float(top[r] - top[r + 1]), False))
                    continue
                both_inf = top[r] == -np.inf
                self._zero("rank", both_inf or cand(ra, ta) == cand(rb, tb))
                ev.add("tie:-inf" if both_inf else "tie:row" if ja == jb else "tie:beams")
                if ja < jb and ta > tb and not both_inf:
                    ev.add("tie:lower-beam-over-lower-token")
                if r == k - 1:
                    ev.add("tie:rank-k")
                if r == 2 * k - 1:
                    ev.add("tie:rank-2k")
                if not both_inf and (ta == self.eos) != (tb == self.eos):
                    ev.add("eos:tie-ahead" if ta == self.eos else "eos:tie-behind")
            nb = n_eos = 0
            for rank in range(2 * k):
                c = int(order[rank])
                j, tok = divmod(c, V)
                if tok == self.eos:
                    n_eos += 1
                    if rank >= k and self.fault != "eos_low":
                        ev.add("eos:rank>=k-skipped")
                        continue
                    ev.add("eos:rank<k-added")
                    self._add(g, flat[c] / cur_len ** self.lp, t, g * k + j, cand(g * k + j, tok))
                else:
                    r = g * k + nb
                    parents[r], tokens[r], new[r], sid[r] = g * k + j, tok, flat[c], cand(g * k + j, tok)
                    if flat[c] == -np.inf:
                        ev.add("ban:-inf-carried")
                    nb += 1
                if nb == k:
                    break
            assert nb == k
            if n_eos > 1:
                ev.add("eos:several-in-a-step")
            if len(self.hyps[g]) >= k:
                best = top[0] / cur_len ** self.lp
                if self.worst[g] == best:                       # by design only when the best candidate IS the worst hypothesis
                    c0 = divmod(int(order[0]), V)
                    low = [self.hsid[g][i] for i, e in enumerate(self.hyps[g]) if e[0] == self.worst[g]]
                    self._zero("done", cand(g * k + c0[0], c0[1]) in low)
                    ev.add("done:at-equality")
                elif best == best:
                    self.gaps.append(("done", abs(self.worst[g] - best), False))
                    if self.worst[g] < best:
                        ev.add("done:missed-by-a-gap")
                self.done[g] = self.worst[g] > best if self.fault == "done_gt" else self.worst[g] >= best
        self.scores, self.sid = new, sid
        if self.strict is not None:
            self.prev = [int(v) for v in tokens]
        self.bp.append((parents, tokens))
        return parents, tokens, new

    def finalize(self, T, max_length):
        if not any(self.done):
            self.events.add("end:no-group-done")
        if T == max_length:
            self.events.add("end:max-length-steps")
        for g in range(self.G):
            if self.done[g]:
                continue
            for j in range(self.k):
                r = g * self.k + j
                self._add(g, self.scores[r] / (1 + T) ** self.lp, T, r, hash((self.sid[r], "running")))
        best = []
        for g, h in enumerate(self.hyps):
            srt = sorted(e[0] for e in h if e[0] == e[0])
            top = srt[-1] if srt else float("nan")
            tied = [i for i, e in enumerate(h) if e[0] == top] or [0]
            if len(tied) > 1:
                self._zero("best", len({self.hsid[g][i] for i in tied}) == 1)
                self.events.add("end:equal-best")
            elif len(srt) > 1:
                self.gaps.append(("best", srt[-1] - srt[-2], False))
            b = 0
            for i in range(1, len(h)):                                     # tests/beam_ref.py's scan (the first for the last: the fault)
                if (h[i][0] > h[b][0]) if self.fault == "best_first" else (h[i][0] >= h[b][0]):
                    b = i
            best.append(h[b])
        seqs = [self.history(e, r) for _, e, r in best]
        W = min(max(len(q) for q in seqs) + 1, 1 + max_length)
        out = np.full((self.G, W), self.pad, dtype=np.int64)
        for g, q in enumerate(seqs):
            out[g, :len(q)] = q
            if len(q) < 1 + max_length:
                out[g, len(q)] = self.eos
        return out, best


def check_margins(what, gaps, err):
    """Every decision gap of the reference is exactly 0 and a designed tie, or larger than max(1e-5, 2 x the score error)."""
    need = max(1e-5, 2 * err)
    bad = [g for g in gaps if g[1] == g[1] and ((g[1] == 0 and not g[2]) or 0 < g[1] <= need)]
    assert not bad, "%s: %d of %d decision gaps are neither a designed tie nor above %.3e: %s" % (what, len(bad), len(gaps), need, bad[:6])
    return min([g[1] for g in gaps if g[1] > 0] or [float("inf")])


def beam_trace(p, lp, ban=None, T=None, copy=None, cls=BeamRef, design=True, **kw):
    """The search of probe p (k beams x G groups) for T steps by `cls` on the design (or on `copy` [rows, T, V]) -> per step
    parents / tokens / scores [T, rows], hypothesis lists and done flags, polls [T, 3], the design's logits; after finalize
    ids [G, W], best, the per-token log-probabilities out_logp [G, W] (float64) and the raw score of each chosen hypothesis."""
    T = T or p.T
    ref = cls(p.G, p.k, p.V, eos=EOS, pad=PAD, start=START, length_penalty=lp, ban=None if ban is None else np.flatnonzero(ban).tolist(), **kw)
    tok = np.full(p.B, START, dtype=np.int64)
    r = SimpleNamespace(parents=[], tokens=[], scores=[], hyps=[], done=[], polls=[], logits=[], lsm=[], ref=ref)
    fin = -1
    for t in range(T):
        lg = design_logits(p, tok, t) if design else copy[:, t].double()
        use = (lg if copy is None else copy[:, t].double()).numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            par, tok, sc = ref.step(t, use)
            r.lsm.append(torch.log_softmax(torch.from_numpy(use), -1).numpy())
        if ref.all_done and fin < 0:
            fin = t
        r.parents.append(par.copy()), r.tokens.append(tok.copy()), r.scores.append(sc.copy()), r.logits.append(lg)
        r.hyps.append([list(h) for h in ref.hyps]), r.done.append(list(ref.done)), r.polls.append((t + 1, int(fin >= 0), fin))
    r.logits = torch.stack(r.logits, 1)
    r.ids, r.best = ref.finalize(T, T)
    r.final_hyps = [list(h) for h in ref.hyps]
    r.out_logp = np.zeros(r.ids.shape)
    r.raw = np.zeros(p.G)
    for g, (_, end, row) in enumerate(r.best):
        e = min(end, T)
        if end < T and 1 + e < r.ids.shape[1]:
            r.out_logp[g, 1 + e] = r.lsm[end][row, EOS]           # the closing EOS, after the prefix row `row` held at step `end`
        for s in range(e - 1, -1, -1):
            par, tk = ref.bp[s]
            r.out_logp[g, s + 1] = r.lsm[s][par[row], tk[row]]
            row = int(par[row])
        r.raw[g] = r.out_logp[g].sum()
    return r


# (id, k, groups, V, steps, length penalty, ban, bf16, seed).  A seed is kept when every decision gap of its float64 search is a
# designed tie or clears 4 x beam_tol of the largest score (tests/test_exact_tail_cpu.py asserts 2 x); among those the one
# that reaches the most scenarios.  The union over the cases is the ledger `BEAM_SCENARIOS`.
BEAM = [
    ("k1-g1-v40-f32", 1, 1, 40, 16, 1.0, None, False, 189),
    ("k1-g1-v1491-ban-bf16", 1, 1, 1491, 16, 0.4, "some", True, 10),
    ("k2-g3-v1491-bf16", 2, 3, 1491, 16, 0.4, None, True, 30),
    ("k2-g3-v1491-f32", 2, 3, 1491, 16, 1.0, None, False, 167),
    ("k3-g3-v1536-bf16-mfma", 3, 3, 1536, 24, 1.0, None, True, 0),
    ("k3-g3-v40-ban-bf16-mfma", 3, 3, 40, 16, 0.4, "some", True, 13),
    ("k8-g2-v1536-bf16-mfma", 8, 2, 1536, 16, 0.4, None, True, 52),
    ("k8-g1-v1491-ban-f32", 8, 1, 1491, 16, 1.0, "some", False, 167),
    ("k2-g3-v40-eos-only-bf16", 2, 3, 40, 16, 1.0, "eos-only", True, 0),
    ("k2-g3-v40-eos-only-f32", 2, 3, 40, 16, 0.4, "eos-only", False, 0),
    ("k2-g2-v40-nan-bf16", 2, 2, 40, 16, 1.0, "nan", True, 3),
    ("k8-g1-v2048-bf16", 8, 1, 2048, 16, 1.0, None, True, 61),
]
BEAM_BIG = ("k8-g32-v1536-bf16-mfma", 8, 32, 1536, 16, 1.0, None, True, 22)
BEAM_SCENARIOS = {"tie:row", "tie:beams", "tie:lower-beam-over-lower-token", "tie:rank-k", "tie:rank-2k", "tie:-inf", "eos:rank<k-added",
                  "eos:rank>=k-skipped", "eos:tie-ahead", "eos:tie-behind", "eos:several-in-a-step", "hyp:overflow",
                  "hyp:overflow-equal-lowest", "end:equal-best", "done:at-equality", "done:missed-by-a-gap",
                  "group:done-while-others-run", "ban:fewer-than-2k-live", "ban:-inf-carried", "nan:row", "end:no-group-done",
                  "end:max-length-steps"}


def beam_case(case):
    """-> (probe, ban mask or None) of a BEAM entry."""
    tag, k, G, V, T, lp, ban, bf16, seed = case
    p = beam_design(V, k, G, T, seed, nan_last=ban == "nan") if bf16 else beam_design_f32(V, k, G, T, seed)
    return p, (beam_ban(p, ban) if ban in ("some", "eos-only") else None)


# ---- what the device leaves behind, and its comparison with a trace ---------------------------------------------------------------

HREC, HYP0 = 32, 4                                   # the hypothesis record of include/mrmt3_hip.h: int32 [groups][32]


def _f32_bits(v):
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


def hyp_records(lists, done, lens=None):
    """[G, 32] int32 records of hypothesis lists [(score, end, row)] (field [1], the worst kept score, is not compared)."""
    rec = np.zeros((len(lists), HREC), dtype=np.int32)
    for g, h in enumerate(lists):
        rec[g, 0], rec[g, 2] = len(h), int(done[g])
        if lens is not None:
            rec[g, 3] = lens[g]
        for i, (s, e, r) in enumerate(h):
            rec[g, HYP0 + 3 * i:HYP0 + 3 * i + 3] = (_f32_bits(s), e, r)
    return rec


def beam_as_device(tr, ld):
    """A trace in the layout the device tests read back (the CPU proof feeds faulty emulations through the same checker)."""
    T, G = len(tr.parents), len(tr.best)
    ids = np.full((G, ld), PAD, dtype=np.int64)
    ids[:, :tr.ids.shape[1]] = tr.ids
    logp = np.zeros((G, ld))
    logp[:, :tr.out_logp.shape[1]] = tr.out_logp
    lens = [len(tr.ref.history(e, r)) for _, e, r in tr.best]
    return SimpleNamespace(bp=torch.from_numpy(np.stack([np.stack(tr.parents), np.stack(tr.tokens)], -1)).int(),
                           tokens=torch.from_numpy(np.stack(tr.tokens, 1)), scores=torch.from_numpy(np.stack(tr.scores)).float(),
                           hyps=torch.from_numpy(np.stack([hyp_records(h, d) for h, d in zip(tr.hyps, tr.done)])),
                           polls=torch.tensor(tr.polls).int(), ids=torch.from_numpy(ids), out_logp=torch.from_numpy(logp).float(),
                           final_hyps=torch.from_numpy(hyp_records(tr.final_hyps, tr.done[-1], lens)))


def _scores_close(what, got, want):
    """NaN and +-inf as themselves, numbers within beam_tol of the reference.  -> the largest error."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    check_within(what, got.reshape(1, 1, -1), want.reshape(1, 1, -1), torch.from_numpy(beam_tol(torch.nan_to_num(
        want, nan=0.0, posinf=0.0, neginf=0.0).numpy())).reshape(1, 1, -1))
    ok = torch.isfinite(want)
    return float((got[ok] - want[ok]).abs().max()) if bool(ok.any()) else 0.0


def _hyps_close(what, rec, lists, done, k):
    rec = torch.as_tensor(rec)
    err = 0.0
    for g, h in enumerate(lists):
        n = int(rec[g, 0])
        got = [(float(rec[g, HYP0 + 3 * i:HYP0 + 3 * i + 1].view(torch.float32)), int(rec[g, HYP0 + 3 * i + 1]), int(rec[g, HYP0 + 3 * i + 2]))
               for i in range(min(n, k + 1))]
        assert n == len(h) and [e[1:] for e in got] == [tuple(e[1:]) for e in h], "%s group %d: records %s, want %s" % (what, g, got, h)
        assert int(rec[g, 2]) == int(done[g]), "%s group %d: done flag %d" % (what, g, int(rec[g, 2]))
        if h:
            err = max(err, _scores_close("%s group %d scores" % (what, g), [e[0] for e in got], [e[0] for e in h]))
    return err


def check_beam(what, got, tr, k, finalize=True):
    """Every step of the device (or of a faulty emulation) against the trace: backpointers, tokens, beam scores, hypothesis
    records in list order, poll triples; then the finalized ids, lengths and log-probabilities.  -> the largest score error."""
    T = len(tr.parents)
    want_bp = torch.from_numpy(np.stack([np.stack(tr.parents), np.stack(tr.tokens)], -1)).int()
    ed.check_equal(what + " backptr (step, row, parent | token)", got.bp[:T], want_bp)
    ed.check_equal(what + " tokens_out", got.tokens[:, :T, None], torch.from_numpy(np.stack(tr.tokens, 1))[..., None])
    ed.check_equal(what + " poll (step, field)", got.polls[:T, :, None].int(), torch.tensor(tr.polls)[..., None].int())
    err = 0.0
    for t in range(T):
        err = max(err, _scores_close("%s beam_scores step %d" % (what, t), got.scores[t], tr.scores[t]))
        err = max(err, _hyps_close("%s hypotheses step %d" % (what, t), got.hyps[t], tr.hyps[t], tr.done[t], k))
    if not finalize:
        return err
    W = tr.ids.shape[1]
    ed.check_equal(what + " out_ids", got.ids[:, :W, None], torch.from_numpy(tr.ids)[..., None])
    assert bool((got.ids[:, W:] == PAD).all()), what + ": out_ids past the output width is not pad"
    err = max(err, _hyps_close(what + " hypotheses after finalize", got.final_hyps, tr.final_hyps, tr.done[-1], k))
    for g, (_, e, r) in enumerate(tr.best):
        assert int(got.final_hyps[g, 3]) == len(tr.ref.history(e, r)), (what, g)
        want = np.zeros(got.out_logp.shape[1])
        want[:W] = tr.out_logp[g]
        _scores_close("%s out_logp group %d" % (what, g), got.out_logp[g], want)
        _scores_close("%s sum of out_logp group %d" % (what, g), [float(got.out_logp[g].double().sum())], [tr.raw[g]])
    return err


# ---- d. the KV-cache reorder: two-layer probes that read the cache back ------------------------------------------------------------
# 512 dimensions: token class (16, +-1 code of token % 16), position (32), the two positions the step reads (32 + 32: `fresh` = t - 1
# and an older one), 8 row bits (injected by layer 0's cross-attention), 8 constants, 384 read-out dimensions.  Both layers
# project q from the two read codes, k from the position code (Hadamard rows: the query's two keys win by 32 c^2 >= 128 nats)
# and v as a selection of the coded dimensions in which every group of four consecutive elements (16 bytes of an f32 row, half
# a 16-byte slot of a bf16 row) holds the three low row bits: any two rows of a beam group differ in every slot.  The read layer's
# w_o_self copies o = (V[fresh] + V[old]) / 2 onto the read-out dimensions, identity lm_head rows show them as banned logit
# columns, a pilot column shows the scale.  Layer 0 is normed before the row bits arrive, so its cache is unique per history
# (token class, position) and not per row.  The driver columns are small random integers of token class, position and row bits.

R_TOK, R_POS, R_SA, R_SB, R_ROW, R_CON, R_READ = 0, 16, 48, 80, 112, 120, 128
R_DRV = 48                                          # driver columns; then 384 read-out columns and the pilot
R_V = R_DRV + INNER + 1
R_STEPS = 28
R_EDGES = (5, 6, 10, 11, 15, 16, 21, 22)            # first / last positions of the 8 KB chunks (768 and 1536 bytes a position)


def _hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def reorder_reads(T):
    """(fresh, old) per step: fresh = t - 1; old visits the chunk edges at an age of >= 3 steps, then cycles."""
    fresh, old, todo = [0] + list(range(T - 1)), [0, 0], list(R_EDGES)
    for t in range(2, T):
        ready = [s for s in todo if s <= t - 3]
        if ready:
            todo.remove(ready[0])
            old.append(ready[0])
        else:
            old.append((5 * t + 1) % (t - 1))
    return fresh, old


def reorder_probe(k, G, read_layer, seed, T=R_STEPS):
    rng = np.random.default_rng([k, G, read_layer, seed, 77])
    B = k * G
    p = SimpleNamespace(B=B, T=T, V=R_V, Lc=1, k=k, G=G, read_layer=read_layer)
    z = lambda *s: torch.zeros(*s, dtype=F64)
    H32 = _hadamard(32)
    wqkv = np.zeros((3 * INNER, D))
    for h in range(6):
        for d in range(1, 32):
            wqkv[h * 64 + d, R_SA:R_SA + 32] = H32[:, d] / 2
            wqkv[h * 64 + d, R_SB:R_SB + 32] = H32[:, d] / 2
            wqkv[INNER + h * 64 + d, R_POS:R_POS + 32] = H32[:, d] / 2
    extra = [R_ROW + b for b in range(3, 8)] + [R_TOK + c for c in range(16)] + [R_POS + s for s in range(32)]
    p.vdims = np.array([R_ROW + j % 4 if j % 4 < 3 else extra[(j // 4) % len(extra)] for j in range(INNER)])
    wqkv[2 * INNER + np.arange(INNER), p.vdims] = 1
    p.layers = []
    for l in range(2):
        w = dict(ln_self=torch.ones(D, dtype=F64), w_qkv=torch.from_numpy(wqkv.copy()), w_o_self=z(D, INNER),
                 ln_cross=torch.ones(D, dtype=F64), w_q_cross=z(INNER, D), w_o_cross=z(D, INNER), ln_ff=torch.ones(D, dtype=F64),
                 w_wi=z(2 * ed.DFF, D), w_wo=z(D, ed.DFF))
        if l == read_layer:
            w["w_o_self"][R_READ + torch.arange(INNER), torch.arange(INNER)] = 1
        if l == 0:
            w["w_o_cross"][R_ROW + torch.arange(8), torch.arange(8)] = 1
        p.layers.append(w)
    lm = np.zeros((R_V, D))
    lm[:R_DRV, R_TOK:R_TOK + 16] = rng.integers(0, 3, (R_DRV, 16))
    lm[:R_DRV, R_POS:R_POS + 32] = rng.integers(0, 3, (R_DRV, 32))
    nb = 3 if G > 8 else 8                                               # 32 groups: one driver for all (8 x fewer distinct gaps)
    lm[:R_DRV, R_ROW:R_ROW + nb] = rng.integers(-2, 3, (R_DRV, nb))
    lm[:R_DRV, R_CON] = np.arange(R_DRV) / 64.0                           # no two columns of a row alike: nothing ties, f32 included
    lm[:R_DRV, R_CON + 1:R_CON + 8] = 9                                   # the driver columns stand well above the read-out columns
    lm[EOS, :] = 0
    lm[EOS, R_CON:R_CON + 8] = -16                                        # EOS never ranks: no group finishes, every step reorders
    lm[R_DRV + np.arange(INNER), R_READ + np.arange(INNER)] = 1
    lm[R_V - 1, R_CON] = 1                                                # the pilot
    p.w = dict(lm_head=torch.from_numpy(lm), final_ln=torch.ones(D, dtype=F64))
    p.bits = np.array([[1.0 if (r >> b) & 1 else -1.0 for b in range(8)] for r in range(B)])
    p.ck = z(2, B, 1, INNER)
    p.cv = z(2, B, 1, INNER)
    p.cv[0, :, 0, :8] = torch.from_numpy(p.bits)
    embed = np.zeros((R_DRV, D))
    embed[:, R_TOK:R_TOK + 16] = _code(np.arange(R_DRV) % 16, 16)
    p.fresh, p.old = reorder_reads(T)
    pos = np.zeros((T + 2, D))
    pos[:, R_POS:R_POS + 32] = pos[:, R_SA:R_SA + 32] = pos[:, R_SB:R_SB + 32] = -1
    for t in range(T):
        pos[t, R_POS + t], pos[t, R_SA + p.fresh[t]], pos[t, R_SB + p.old[t]] = 1, 1, 1
    pos[:, R_CON:R_CON + 8] = 1
    p.embed, p.pos = torch.from_numpy(np.vstack([embed, np.zeros((R_V - R_DRV, D))])), torch.from_numpy(pos)
    p.ban = np.arange(R_V) >= R_DRV
    return p


def check_reorder_probe(p):
    for w in p.layers + [p.w]:
        for name, t in w.items():
            assert torch.equal(ed._bf16(t), t), name
    for t in (p.ck, p.cv, p.embed, p.pos):
        assert torch.equal(ed._bf16(t), t)
    assert p.T * INNER * 2 > 2 * 8192 and (p.T * INNER * 2) % 8192 and (p.T * INNER * 4) % 8192      # two boundaries, a partial chunk
    for g0 in range(0, p.B, p.k):                                          # every 4 elements tell any two rows of a group apart
        rows = p.bits[g0:g0 + p.k, :3]
        assert len({tuple(r) for r in rows}) == p.k
    assert all((p.vdims[j:j + 3] == R_ROW + np.arange(3)).all() for j in range(0, INNER, 4))
    visited = set(p.fresh) | set(p.old)
    assert visited >= set(range(p.T - 1))
    for s in R_EDGES:
        assert any(p.old[t] == s and t - s >= 3 for t in range(p.T)), s


REORDER_FAULTS = ("swap_overwrite", "slot_sibling", "skip_last_chunk", "kv_exchanged", "layer1_prev_map")


def reorder_emulate(p, bf16, fault=None, lp=1.0):
    """The two-layer step with explicit caches and the reorder after every select, in float64 (bf16 = True rounds where a bf16
    handle rounds).  -> logits [rows, T, V]; with `fault` the reorder of the read layer goes wrong in one way."""
    rnd = (lambda a: ed._bf16(torch.from_numpy(a)).numpy()) if bf16 else (lambda a: a)
    B, T, k = p.B, p.T, p.k
    ref = BeamRef(p.G, k, p.V, eos=EOS, pad=PAD, start=START, length_penalty=lp, ban=np.flatnonzero(p.ban).tolist())
    W = [{n: t.numpy() for n, t in w.items()} for w in p.layers]
    lm, emb, pos = p.w["lm_head"].numpy(), p.embed.numpy(), p.pos.numpy()
    Kc, Vc = np.zeros((2, B, T, INNER)), np.zeros((2, B, T, INNER))
    tok, out, prev_par = np.full(B, START), [], np.arange(B)
    esz = 2 if bf16 else 4
    norm = lambda x: rnd(x / np.sqrt((x * x).mean(-1, keepdims=True) + ed.EPS))
    for t in range(T):
        x = emb[tok] + pos[t]
        for l in range(2):
            q, kk, v = np.split(norm(x) @ W[l]["w_qkv"].T, 3, -1)
            Kc[l][:, t], Vc[l][:, t] = rnd(kk), rnd(v)
            sc = np.einsum("bhd,bshd->bhs", q.reshape(B, 6, 64), Kc[l][:, :t + 1].reshape(B, t + 1, 6, 64))
            pr = np.exp(sc - sc.max(-1, keepdims=True))
            pr /= pr.sum(-1, keepdims=True)
            o = np.einsum("bhs,bshd->bhd", pr, Vc[l][:, :t + 1].reshape(B, t + 1, 6, 64)).reshape(B, INNER)
            x = x + rnd(o) @ W[l]["w_o_self"].T
            if l == 0:
                x[:, R_ROW:R_ROW + 8] += p.bits
        lg = norm(x) @ lm.T
        out.append(lg)
        par, tok, _ = ref.step(t, lg)
        for l in range(2):
            use = prev_par if (fault == "layer1_prev_map" and l == 1) else par
            oldK, oldV = Kc[l].copy(), Vc[l].copy()
            if fault == "swap_overwrite" and l == p.read_layer:
                for r in range(B):                                       # in place, row after row: a parent may be gone already
                    Kc[l][r], Vc[l][r] = Kc[l][use[r]].copy(), Vc[l][use[r]].copy()
            elif fault == "kv_exchanged" and l == p.read_layer:
                moved = use != np.arange(B)
                Kc[l][moved], Vc[l][moved] = oldV[use][moved], oldK[use][moved]
            else:
                Kc[l], Vc[l] = oldK[use], oldV[use]
            if l == p.read_layer and fault == "slot_sibling":
                n = 16 // esz
                for r in np.flatnonzero(use != np.arange(B)):
                    sib = (use[r] // k) * k + (use[r] % k + 1) % k
                    Vc[l][r, :t + 1, 3 * n:4 * n] = oldV[sib, :t + 1, 3 * n:4 * n]
            if l == p.read_layer and fault == "skip_last_chunk":
                per = 8192 // esz
                first = ((t + 1) * INNER // per) * per                    # element index where the last, partial chunk begins
                fk, fv = Kc[l].reshape(B, -1), Vc[l].reshape(B, -1)
                live = slice(first, (t + 1) * INNER)
                fk[:, live], fv[:, live] = oldK.reshape(B, -1)[:, live], oldV.reshape(B, -1)[:, live]
        prev_par = par
    return torch.from_numpy(np.stack(out, 1))


def reorder_scale(p, bf16):
    """What one unit of the read layer's V is: rstd of its self-attention norm (120 or 128 coded dimensions of +-1 among 512)."""
    n = 128 if p.read_layer == 1 else 120
    c = torch.tensor(1.0 / np.sqrt(n / 512.0 + ed.EPS), dtype=F64)
    return float(ed._bf16(c)) if bf16 else float(c)


def reorder_expected(p, tr):
    """[rows, T, 384] in units of V: (code of holder(r, fresh(t)) + code of holder(r, old(t))) / 2, the holders followed through
    the reference's backpointers; the code of (row h, token it was fed, position s) is the coded residual at `vdims`."""
    B, T = p.B, p.T
    tokin = [np.full(B, START)] + [np.asarray(tk) for tk in tr.tokens[:-1]]
    emb, pos = p.embed.numpy(), p.pos.numpy()

    def code(h, s):
        x = emb[tokin[s][h]] + pos[s]
        if p.read_layer == 1:
            x[:, R_ROW:R_ROW + 8] += p.bits[h]
        return x[:, p.vdims]

    want = np.zeros((B, T, INNER))
    for t in range(T):
        anc = {t: np.arange(B)}
        for s in range(t - 1, -1, -1):
            anc[s] = np.asarray(tr.parents[s])[anc[s + 1]]
        want[:, t] = (code(anc[p.fresh[t]], p.fresh[t]) + code(anc[p.old[t]], p.old[t])) / 2
    return torch.from_numpy(want)


def check_reorder(what, p, logits, bf16, bp=None, lp=1.0):
    """The device's (or a faulty emulation's) logits [rows, T, V]: tests/beam_ref.py on them gives the backpointers (compared with
    the device's `bp` [T, rows, 2] when given); the read-out columns, in units of V, must be the closed form within ATTN_TOL."""
    tr = beam_trace(p, lp, p.ban, copy=logits, design=False)
    if bp is not None:
        want = torch.from_numpy(np.stack([np.stack(tr.parents), np.stack(tr.tokens)], -1)).int()
        ed.check_equal(what + " backptr (step, row, parent | token)", bp[:p.T], want)
    lg = logits.double()
    units = lg[..., R_DRV:R_DRV + INNER] / lg[..., -1:] / reorder_scale(p, bf16)
    want = reorder_expected(p, tr)
    assert 0.5 >= 4 * ed.ex.ATTN_TOL                                       # the smallest fault step: one of two +-1 against a 0
    return ed.check_within(what + " read-out", units, want, ed.ex.ATTN_TOL), tr


def reorder_ledger(p, tr):
    """The parent maps the reference's search produces, per (step, group)."""
    out, k = set(), p.k
    for par in tr.parents:
        for g in range(p.G):
            m = np.asarray(par[g * k:(g + 1) * k]) - g * k
            if (m == np.arange(k)).all():
                out.add("identity")
            if any(m[i] == j and m[j] == i for i in range(k) for j in range(i + 1, k)):
                out.add("swap")
            if any(len({i, m[i], m[m[i]]}) == 3 and m[m[m[i]]] == i for i in range(k)):
                out.add("3-cycle")
            if len(set(m)) == 1 and k > 1:
                out.add("fan-out")
            if k == 8 and (m != np.arange(k)).all():
                out.add("all-moved-k8")
    return out


# (id, k, groups, read layer, bf16, seed): seeds searched on the emulation for clear margins; the ledger is the union over the cases
REORDER = [
    ("read1-k3-g3-bf16", 3, 3, 1, True, 0),
    ("read1-k3-g3-f32", 3, 3, 1, False, 0),
    ("read1-k8-g3-bf16", 8, 3, 1, True, 8),
    ("read1-k8-g3-f32", 8, 3, 1, False, 35),
    ("read0-k3-g3-f32", 3, 3, 0, False, 2),
    ("read0-k8-g3-bf16", 8, 3, 0, True, 25),
]
REORDER_BIG = [("read1-k8-g32-bf16", 8, 32, 1, True, 3), ("read0-k8-g32-bf16", 8, 32, 0, True, 0)]
REORDER_MAPS = {"identity", "swap", "3-cycle", "fan-out", "all-moved-k8"}
