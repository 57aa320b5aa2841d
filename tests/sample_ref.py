"""TEST INFRASTRUCTURE ONLY: host restatement of the decoder's sampling rule (csrc/decode_tail.hip `sample_draw`), next
to tests/beam_ref.py.  float64 over given f32 logits; nothing here shares code with the kernel.

The rule, per row (HF 4.18 `sample()`: NoBadWords -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
multinomial):
  1. banned logits -> -inf;
  2. s = l / T, the f32 quotient (T == 1: the bits as they are);
  3. top_k > 0: every s strictly below the min(top_k, V)-th largest is removed, ties with it stay;
  4. top_p < 1 (its f32 value): token c stays iff the softmax mass of the tokens with a strictly larger s is <= top_p;
  5. the token is the lowest index whose cumulative kept probability, in ascending index, exceeds u; a draw that rounding
     puts past the last kept token takes that token.
`u` = 24 bits / 2^24 from two `drop_mix` rounds over the counter (row, step).
A row that holds an unbanned NaN, or whose maximum is not finite, is `greedy`: the kernel emits torch.argmax's token.
"""
import numpy as np

from oracle.dropout_ref import drop_mix

M32 = 0xFFFFFFFF
SLACK = 2e-5


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & M32) ^ (((seed >> 32) * 0x9E3779B1) & M32)


def u24(seed, row, step):
    """24 random bits of every (row, step) pair; `row` and `step` broadcast against each other."""
    row = np.asarray(row, dtype=np.uint64)
    step = np.asarray(step, dtype=np.uint64)
    m = np.uint64(M32)
    a = drop_mix((np.uint64(seed_key(seed)) + row * np.uint64(0x9E3779B1) + step * np.uint64(0xC2B2AE35)) & m)
    h = drop_mix((a + step * np.uint64(0x85EBCA6B) + row * np.uint64(0x27D4EB2F) + np.uint64(0x7F4A7C15)) & m)
    return (h >> np.uint64(8)).astype(np.int64)


def uniform(seed, row, step):
    return u24(seed, row, step).astype(np.float64) / float(1 << 24)


class Rows:
    """kept [R, V] bool; lo, hi [R, V] f64: token c owns [lo, hi) of the normalised cumulative probability (lo == hi where
    it is not kept); greedy [R] bool and greedy_token [R]: rows the rule does not draw from."""

    def __init__(self, kept, lo, hi, greedy, greedy_token):
        self.kept, self.lo, self.hi, self.greedy, self.greedy_token = kept, lo, hi, greedy, greedy_token

    def pick(self, u):
        """The host's token per row for draws u [R]."""
        above = self.kept & (self.hi > u[:, None])
        first = np.argmax(above, 1)
        last = self.kept.shape[1] - 1 - np.argmax(self.kept[:, ::-1], 1)
        tok = np.where(above.any(1), first, last)
        return np.where(self.greedy, self.greedy_token, tok)

    def edge_distance(self, u):
        """min over the interior interval edges of |u - edge| per row (inf for greedy rows and one-token rows)."""
        edges = np.where(self.kept & (self.hi < 1.0 - 1e-15), self.hi, np.inf)
        d = np.abs(edges - u[:, None]).min(1)
        return np.where(self.greedy, np.inf, d)

    def check(self, tokens, u, slack=SLACK):
        """-> (wrong [R] bool, by_slack [R] bool): a token is right when it is kept and its interval holds u within
        `slack`; it is right `by_slack` when only the slack makes it so."""
        tokens = np.asarray(tokens)
        r = np.arange(len(tokens))
        inb = (tokens >= 0) & (tokens < self.kept.shape[1])
        t = np.where(inb, tokens, 0)
        lo, hi, kept = self.lo[r, t], self.hi[r, t], self.kept[r, t] & inb
        last = self.kept.shape[1] - 1 - np.argmax(self.kept[:, ::-1], 1)
        exact = kept & (lo <= u) & ((u < hi) | (t == last))
        loose = kept & (lo - slack <= u) & ((u < hi + slack) | (t == last))
        g_ok = tokens == self.greedy_token
        wrong = np.where(self.greedy, ~g_ok, ~loose)
        return wrong, np.where(self.greedy, False, loose & ~exact)


def torch_argmax(x):
    """torch.argmax of a 2-D f32 array: the first NaN, else the first maximum."""
    nan = np.isnan(x)
    return np.where(nan.any(1), np.argmax(nan, 1), np.argmax(np.where(nan, -np.inf, x), 1))


def sample_ref(logits, ban=None, temperature=1.0, top_k=0, top_p=1.0):
    """logits [R, V] f32 (numpy); `ban`: indices or a [V] mask.  -> Rows."""
    l = np.array(logits, dtype=np.float32, copy=True)
    R, V = l.shape
    if ban is not None:
        b = np.asarray(ban)
        l[:, np.flatnonzero(b) if b.dtype in (np.bool_, np.uint8) and b.shape == (V,) else b.astype(np.int64)] = -np.inf
    greedy_token = torch_argmax(l)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.where(np.isnan(l).any(1), np.nan, np.max(np.where(np.isnan(l), -np.inf, l), 1))
        greedy = ~np.isfinite(mx)
        s32 = l if float(temperature) == 1.0 else (l / np.float32(temperature)).astype(np.float32)
        s = np.where(greedy[:, None], 0.0, s32.astype(np.float64))          # greedy rows: a harmless stand-in
        s = np.where(np.isnan(s), 0.0, s)
        kept = np.ones((R, V), dtype=bool)
        if top_k > 0 and top_k < V:
            kth = np.sort(s, 1)[:, V - top_k]
            kept &= s >= kth[:, None]
        e = np.where(kept, np.exp(s - s.max(1, keepdims=True)), 0.0)
        if top_p < 1.0:
            order = np.argsort(-s, 1, kind="stable")
            ss, es = np.take_along_axis(s, order, 1), np.take_along_axis(e, order, 1)
            before = np.cumsum(es, 1) - es                                   # mass ahead of each sorted position
            new = np.concatenate([np.ones((R, 1), bool), ss[:, 1:] != ss[:, :-1]], 1)
            first = np.maximum.accumulate(np.where(new, np.arange(V)[None, :], 0), 1)   # where the tie group starts
            above = np.take_along_axis(before, first, 1)
            keep_sorted = above <= np.float64(np.float32(top_p)) * es.sum(1, keepdims=True)
            kp = np.zeros((R, V), dtype=bool)
            np.put_along_axis(kp, order, keep_sorted, 1)
            kept &= kp
            e = np.where(kept, e, 0.0)
        kept &= e > 0.0                                                      # -inf entries (banned) carry no mass
        Z = e.sum(1, keepdims=True)
        hi = np.cumsum(e, 1) / Z
        lo = np.concatenate([np.zeros((R, 1)), hi[:, :-1]], 1)
    return Rows(kept, lo, hi, greedy, greedy_token)


def hf_kept(logits, temperature, top_k, top_p):
    """HF 4.18's TemperatureLogitsWarper, TopKLogitsWarper and TopPLogitsWarper (min_tokens_to_keep = 1) restated with
    torch in float64, for rows of distinct logits: the kept mask [R, V]."""
    import torch
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32))
    x = (x if float(temperature) == 1.0 else x / torch.tensor(temperature, dtype=torch.float32)).double()
    if top_k > 0:
        k = min(top_k, x.shape[-1])
        x = x.masked_fill(x < torch.topk(x, k)[0][..., -1, None], -float("inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(x, descending=True)
        cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cumulative_probs > float(np.float32(top_p))
        remove[..., 1:] = remove[..., :-1].clone()
        remove[..., 0] = False
        x = x.masked_fill(remove.scatter(1, sorted_indices, remove), -float("inf"))
    return torch.isfinite(x).numpy()


# ---- the standalone-kernel cases of tests/test_sample_gpu.py, built on the host ------------------------------------
# (name, V, rows, kind, ban, temperature, top_k, top_p, seed).  The seeds were searched on this restatement alone so that no
# draw of a case lies within SLACK of an interval edge (tests/test_sample_cpu.py asserts it): the kernel must then return
# the host's token for every row.  That is only possible where rows x kept tokens x 2 SLACK is well below 1, so the
# 4096-row cases are the 8-live-token row and V = 5.
CASE_BAN = list(range(2, 1536, 3))
CASES = [
    ("gauss-v5-r1", 5, 1, "gauss", None, 1.0, 0, 1.0, 1000),
    ("gauss-v64-r8-T.5-k7", 64, 8, "gauss", None, 0.5, 7, 1.0, 2000),
    ("gauss-v65-r9-T2-p.9", 65, 9, "gauss", None, 2.0, 0, 0.9, 3000),
    ("gauss-v65-r9-k7-p.3", 65, 9, "gauss", None, 1.0, 7, 0.3, 4000),
    ("gauss-v1536-r8", 1536, 8, "gauss", None, 1.0, 0, 1.0, 5000),
    ("gauss-v1536-r9-k7-p.9", 1536, 9, "gauss", None, 1.0, 7, 0.9, 6000),
    ("gauss-v2048-r8-T.5-p.3", 2048, 8, "gauss", None, 0.5, 0, 0.3, 7000),
    ("gauss-v2048-r1-T2-k1", 2048, 1, "gauss", None, 2.0, 1, 1.0, 8000),
    ("gauss-v5-r4096-p.9", 5, 4096, "gauss", None, 1.0, 0, 0.9, 9000),
    ("ties-v5-r8-k1", 5, 8, "ties", None, 1.0, 1, 1.0, 10000),
    ("ties-v64-r9-k7-p.9", 64, 9, "ties", None, 1.0, 7, 0.9, 11000),
    ("ties-v1536-r8-T2-k7-p.3", 1536, 8, "ties", None, 2.0, 7, 0.3, 12000),
    ("ban-v1536-r9-p.9", 1536, 9, "gauss", CASE_BAN, 1.0, 0, 0.9, 13000),
    ("ban-v65-r8-T.5-k7", 65, 8, "gauss", [0, 3, 64], 0.5, 7, 1.0, 14000),
    ("live8-v1536-r4096", 1536, 4096, "live8", None, 1.0, 0, 1.0, 15003),
    ("live8-v64-r4096-T2-k7-p.9", 64, 4096, "live8", None, 2.0, 7, 0.9, 16002),
    ("live8-v2048-r4096-T.5-p.3", 2048, 4096, "live8", None, 0.5, 0, 0.3, 17000),
]
CASE_STEP, CASE_ROW0 = 5, 3       # the counter every case draws with: (CASE_ROW0 + r, CASE_STEP)


def case_logits(name, V, rows, kind):
    """The f32 logits of a case, from a generator seeded by the case's shape and kind."""
    g = np.random.default_rng([V, rows, len(kind), sum(map(ord, kind))])
    if kind == "gauss":
        return (2.0 * g.standard_normal((rows, V))).astype(np.float32)
    if kind == "ties":                                    # quarter steps: most values have twins, the maximum often too
        return (np.round(4.0 * g.standard_normal((rows, V))) / 4.0).astype(np.float32)
    assert kind == "live8"
    row = np.full(V, -np.inf, dtype=np.float32)
    cols = np.sort(g.choice(V, size=min(8, V), replace=False))
    row[cols] = (1.5 * g.standard_normal(len(cols))).astype(np.float32)
    return np.repeat(row[None, :], rows, 0)
