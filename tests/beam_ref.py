"""Host restatement (float64) of the beam search the decoder runs on the GPU (csrc/decode_tail.hip dec_beam_select /
dec_beam_finalize_kernel): HF 4.18 `beam_search` + `BeamSearchScorer` with early_stopping=False and one hypothesis kept,
`max_length` counting new tokens.  Used by tests/test_beam_decode_{cpu,gpu}.py; not a test module itself.

Rows r = g * k + j are beam j of group g.  `step(t, logits)` consumes the [G*k, V] logits of token step t and returns
(parents, tokens, scores) per row; `finalize(T, max_length)` returns the [G, W] int64 output.  `margins` collects, per
step, the smallest score gap among the top 2k + 1 candidates of each group (what decides the ranks) and `done_margins`
the gap of every done test and hypothesis admission, so a GPU comparison can assert its fixture is not a near tie."""
import numpy as np


class BeamRef:
    def __init__(self, G, k, V, eos=1, pad=0, start=0, length_penalty=1.0, ban=None):
        self.G, self.k, self.V, self.eos, self.pad, self.start, self.lp = G, k, V, eos, pad, start, length_penalty
        self.ban = None if not ban else np.asarray(sorted(set(ban)), dtype=np.int64)
        self.scores = np.zeros(G * k)
        self.scores.reshape(G, k)[:, 1:] = -1e9
        self.hyps = [[] for _ in range(G)]          # per group, insertion order: (score, end step, row)
        self.worst = [1e9] * G
        self.done = [False] * G
        self.bp = []                                # per step: (parents [G*k], tokens [G*k])
        self.margins = []
        self.done_margins = []

    # BeamHypotheses.add
    def _add(self, g, score, end, row):
        h = self.hyps[g]
        if len(h) < self.k or score > self.worst[g]:
            if len(h) >= self.k:
                self.done_margins.append(abs(score - self.worst[g]))
            h.append((score, end, row))
            if len(h) > self.k:
                srt = sorted([(s, i) for i, (s, _, _) in enumerate(h)])
                del h[srt[0][1]]
                self.worst[g] = srt[1][0]
            else:
                self.worst[g] = min(score, self.worst[g])
        else:
            self.done_margins.append(abs(score - self.worst[g]))

    def step(self, t, logits):
        G, k, V = self.G, self.k, self.V
        x = np.asarray(logits, dtype=np.float64).reshape(G * k, V)
        m = x.max(-1, keepdims=True)
        logp = (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))
        if self.ban is not None:
            logp[:, self.ban] = -np.inf
        s = logp + self.scores[:, None]
        parents = np.arange(G * k)
        tokens = np.full(G * k, self.pad, dtype=np.int64)
        new = np.zeros(G * k)
        cur_len = t + 1
        for g in range(G):
            if self.done[g]:
                continue
            flat = s[g * k:(g + 1) * k].reshape(-1)
            # score descending (a NaN above every number, as torch.topk ranks it), then flat index
            order = np.lexsort((np.arange(flat.size), -flat, ~np.isnan(flat)))[:2 * k + 1]
            top = flat[order]
            fin = top[np.isfinite(top)]
            if len(fin) > 1:
                self.margins.append(float(np.min(fin[:-1] - fin[1:])))
            nb = 0
            for rank in range(2 * k):
                c = int(order[rank])
                j, tok = divmod(c, V)
                if tok == self.eos:
                    if rank >= k:
                        continue
                    self._add(g, flat[c] / cur_len ** self.lp, t, g * k + j)
                else:
                    r = g * k + nb
                    parents[r], tokens[r], new[r] = g * k + j, tok, flat[c]
                    nb += 1
                if nb == k:
                    break
            assert nb == k
            if len(self.hyps[g]) >= k:
                best = top[0] / cur_len ** self.lp
                if self.worst[g] != best:           # equal by construction when the best candidate is the worst hypothesis
                    self.done_margins.append(abs(self.worst[g] - best))
                self.done[g] = self.worst[g] >= best
        self.scores = new
        self.bp.append((parents, tokens))
        return parents, tokens, new

    def history(self, end, row):
        """Start token + row's tokens of steps 0..end-1."""
        out = []
        for s in range(end - 1, -1, -1):
            p, tk = self.bp[s]
            out.append(int(tk[row]))
            row = int(p[row])
        return [self.start] + out[::-1]

    def finalize(self, T, max_length):
        """T = steps run.  Returns (ids [G, W] int64, chosen (score, end, row) per group)."""
        for g in range(self.G):
            if self.done[g]:
                continue
            for j in range(self.k):
                r = g * self.k + j
                self._add(g, self.scores[r] / (1 + T) ** self.lp, T, r)
        best = []
        for h in self.hyps:                     # stable sort + pop(): the last of equal maxima, written as the scan the kernel
            b = 0                               # runs so that a NaN score has a place: it compares false both ways, so the
            for i in range(1, len(h)):          # list's first entry stays chosen if it is NaN and a later NaN never is
                if h[i][0] >= h[b][0]:
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

    @property
    def all_done(self):
        return all(self.done)


def beam_search(logits_fn, G, k, V, max_length, **kw):
    """Full search driven by `logits_fn(t, ids [G*k, t+1]) -> [G*k, V]` (the rows' running sequences, start first)."""
    ref = BeamRef(G, k, V, **kw)
    ids = np.full((G * k, 1), ref.start, dtype=np.int64)
    T = 0
    for t in range(max_length):
        parents, tokens, _ = ref.step(t, logits_fn(t, ids))
        ids = np.concatenate([ids[parents], tokens[:, None]], 1)
        T = t + 1
        if ref.all_done:
            break
    return ref.finalize(T, max_length)[0], ref
