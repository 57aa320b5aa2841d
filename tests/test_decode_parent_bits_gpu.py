"""The KV-cached decoder writes the bits it wrote before csrc/decode.hip was split into decode.hip (handle, per-layer
kernels, the one step launcher), decode_tail.hip (greedy / sampled / beam tails) and decode_grammar.hip (event grammar)
around csrc/decode.h.  The fp64 tests (tests/test_decode_gpu.py and the beam / sample / logprob / grammar files) bound the
arithmetic; a launcher that passed a kernel another grid, LDS size, stride or weight pointer could stay inside those bounds
(or move a step's logits by an ulp), so here every step's logits are compared bit for bit.  tests/golden/decode_parent.json
holds, for each case below, the sha256 of every buffer the decode returns as the PARENT commit (named in the file) wrote it
on an MI355X.

How the golden was recorded: the parent commit's csrc/ was built into a library of its own, a script loaded it in place of
the tree's (MRMT3_TOOL_LIB: the C ABI and the Python binding did not change), ran `run_case(name, dev)` for every name in
CASES and dumped {"parent": <commit>, "cases": {name: result}} as JSON.  Inputs (encoder states, prefix rows, carries) come
from numpy's default_rng on the host; the model is the `t5` variant with the golden weights, cut to two decoder layers.

Every decode runs twice on its handle: the step graph is captured once per tail configuration, the second decode with the
same configuration replays it (capture_count does not move) and returns the same bits.

`test_a_changed_norm_pointer_recaptures` is the one intended behaviour change of that split: see its docstring."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grammar_ref as gr  # noqa: E402
from contrib import vocabularies  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_parent.json")
BF, F32 = torch.bfloat16, torch.float32
CODEC = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
_MODELS = {}


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _model(dtype, dev, layers=2):
    if (dtype, layers) not in _MODELS:
        from mrmt3.synthetic import T5_SMALL
        from models.t5 import T5ForConditionalGeneration
        m = T5ForConditionalGeneration(dict(T5_SMALL, num_decoder_layers=layers), compute_dtype=dtype)
        m = m.load_golden().to(dev).eval()
        m.engine.prepare(False)
        _MODELS[(dtype, layers)] = m
    return _MODELS[(dtype, layers)]


def _enc(rng, m, B, Lc):
    """[B * Lc, d] encoder states in the engine's dtype"""
    x = rng.standard_normal((B * Lc, m.cfg["d_model"])).astype(np.float32)
    return torch.from_numpy(x).to(m.engine.dt).to(m.device)


def _grammar():
    from mrmt3.grammar import EventGrammar
    return EventGrammar.from_codec(CODEC)


def _carry(rng, rows, dev, n=200):
    """[rows, 2048] uint8: n (program, pitch) pairs over four programs per row"""
    out = []
    for _ in range(rows):
        progs = rng.choice(128, size=4, replace=False)
        out.append(gr.set_to_bits({(int(rng.choice(progs)), int(rng.integers(0, 128))) for _ in range(n)}))
    return torch.from_numpy(np.stack(out)).to(dev)


def _twice(dec, decode, captures):
    """`decode()` twice on `dec`: `captures` step graphs afterwards, none of them from the second call; the same bits."""
    first = decode()
    assert dec.graph_captured and dec.capture_count == captures
    again = decode()
    assert dec.graph_captured and dec.capture_count == captures
    assert again == first
    return first


def _run(m, dec, ckv, B, Lc, steps, prefix=None, **kw):
    """dec.run with every step's logits copied out -> hashes of the token rows, the logits and what the mode adds"""
    n_pre = 0 if prefix is None else prefix.shape[1]
    logits = torch.full((n_pre + steps, B, m.cfg["vocab_size"]), float("nan"), device=m.device)
    with torch.no_grad():
        out = dec.run(ckv, B, Lc, steps, prefix=prefix, logits_out=logits, **kw)
        torch.cuda.synchronize()
    assert out[1] == n_pre + steps
    r = {"tokens": _sha(out[0][:B, :steps + 1]), "logits": _sha(logits)}
    if kw.get("return_logprobs"):
        r["logp"] = _sha(out[3][:B, :steps + 1])
    return r, logits


def case_greedy(dev, dtype, B, Lc, steps, n_pre=0):
    """fp32 B = 3, Lc = 250: the gemv <float> kernels, a cross length whose score rows round up to 252 floats of LDS.
    bf16 B = 8: gemv <bf16_t> at the largest batch it takes; B = 9, 17: the MFMA kernels with a ragged group of 16
    sequences (9 of 16; 16 + 1).  n_pre: memory rows ahead of the start token, whose steps pass through the tail."""
    from mrmt3.decode import Decoder
    m = _model(dtype, dev)
    rng = np.random.default_rng(301)
    enc = _enc(rng, m, B, Lc)
    pre = None
    if n_pre:
        pre = torch.from_numpy(rng.standard_normal((B, n_pre, m.cfg["d_model"])).astype(np.float32)).to(dev)
    dec = Decoder(m, B, n_pre + steps, Lc)
    ckv = dec.cross_kv(enc, B, Lc)
    return _twice(dec, lambda: _run(m, dec, ckv, B, Lc, steps, prefix=pre)[0], 1)


def _ban_ids(V):
    return [i for i in range(2, V) if i % 3 == 0]          # a third of the vocabulary; never EOS (1) or the tie token


def case_ban_logp(dev):
    """dec_argmax<true, true>: a static ban and per-token log-probabilities"""
    from mrmt3.decode import Decoder
    m, B, Lc, steps = _model(BF, dev), 9, 256, 12
    enc = _enc(np.random.default_rng(302), m, B, Lc)
    dec = Decoder(m, B, steps, Lc)
    ckv = dec.cross_kv(enc, B, Lc)
    ban = _ban_ids(m.cfg["vocab_size"])
    return _twice(dec, lambda: _run(m, dec, ckv, B, Lc, steps, ban=dec.ban_mask(ban), return_logprobs=True)[0], 1)


def case_sampled(dev):
    """dec_sample<false, true>, and mrmt3_sample_logits on the last step's logits"""
    from mrmt3 import lib
    from mrmt3.decode import Decoder
    m, B, Lc, steps = _model(BF, dev), 9, 256, 12
    enc = _enc(np.random.default_rng(303), m, B, Lc)
    dec = Decoder(m, B, steps, Lc)
    ckv = dec.cross_kv(enc, B, Lc)

    def decode():
        r, logits = _run(m, dec, ckv, B, Lc, steps, sampling=(0.7, 50, 0.9, 20251), return_logprobs=True)
        tok, lp = lib.sample_logits(logits[steps - 1].contiguous(), 0.7, 50, 0.9, seed=20251, step=steps - 1, return_logprobs=True)
        r["alone"] = {"tokens": _sha(tok), "logp": _sha(lp)}
        return r

    return _twice(dec, decode, 1)


def _beam(m, dec, ckv, G, k, Lc, steps, **kw):
    logits = torch.full((steps, G * k, m.cfg["vocab_size"]), float("nan"), device=m.device)
    with torch.no_grad():
        ids, done, fin, lp = dec.run_beam(ckv, G, k, Lc, steps, 0.6, logits_out=logits, return_logprobs=True, **kw)
        torch.cuda.synchronize()
    assert done == steps
    return {"ids": _sha(ids), "logp": _sha(lp), "logits": _sha(logits), "tokens": _sha(dec.tokens[:G * k, :steps + 1]),
            "bp": _sha(dec.backptr(G * k)[:steps]), "scores": _sha(dec.beam_scores(G * k)), "hyps": _sha(dec.hyps(G))}


def case_beam(dev):
    """3 groups x 4 beams under a ban: dec_beam_select, dec_beam_reorder, the finalize kernel with log-probabilities"""
    from mrmt3.decode import Decoder
    m, G, k, Lc, steps = _model(BF, dev), 3, 4, 256, 12
    enc = _enc(np.random.default_rng(304), m, G, Lc)
    dec = Decoder(m, G * k, steps, Lc)
    ckv = dec.cross_kv_beam(enc, G, k, Lc)
    ban = _ban_ids(m.cfg["vocab_size"])
    return _twice(dec, lambda: _beam(m, dec, ckv, G, k, Lc, steps, ban=dec.ban_mask(ban)), 1)


def case_grammar(dev):
    """dec_grammar_step behind the greedy tail (9 rows) and behind beam search (2 x 4), each with a carry: the mask per row
    (ban stride V), the parents' states under reparenting, and the replay kernel of grammar_active"""
    from mrmt3.decode import Decoder
    m, Lc, steps = _model(BF, dev), 256, 12
    rng = np.random.default_rng(305)
    dec = Decoder(m, 9, steps, Lc)
    enc9, enc2 = _enc(rng, m, 9, Lc), _enc(rng, m, 2, Lc)
    carry9 = _carry(rng, 9, dev)
    carry2 = _carry(rng, 2, dev).repeat_interleave(4, 0).contiguous()
    out = {}

    def greedy():
        ckv = dec.cross_kv(enc9, 9, Lc)
        r = _run(m, dec, ckv, 9, Lc, steps, grammar=_grammar(), carry=carry9)[0]
        r["active"] = _sha(dec.grammar_active(9))
        return r

    def beam():
        ckv = dec.cross_kv_beam(enc2, 2, 4, Lc)
        r = _beam(m, dec, ckv, 2, 4, Lc, steps, grammar=_grammar(), carry=carry2)
        r["active"] = _sha(dec.grammar_active(2))
        return r

    out["greedy"] = _twice(dec, greedy, 1)
    out["beam"] = _twice(dec, beam, 2)
    return out


def case_grammar_alone(dev):
    """mrmt3_grammar_init / _advance / _active / _replay on 5 rows (V = 1536) with a carry and a static ban: 40 steps of
    tokens drawn on the host from each row's own mask, rows reparented at every third step, row 4 idle on pad from step 20."""
    from mrmt3 import lib
    rows, V, steps = 5, 1536, 40
    rng = np.random.default_rng(306)
    carry = _carry(rng, rows, dev, n=24)
    ban = torch.zeros(V, dtype=torch.uint8)
    ban[[1135 + 7, 1004 + 60]] = 1
    st = lib.GrammarState(_grammar(), rows, V, dev, carry=carry, ban=ban.to(dev))
    out = {"mask0": _sha(st.mask)}
    ids = np.zeros((rows, steps + 1), dtype=np.int64)
    for s in range(steps):
        par = rng.permutation(rows).astype(np.int32) if s % 3 == 2 else np.arange(rows, dtype=np.int32)
        mask = st.mask.cpu().numpy()
        tok = np.zeros(rows, dtype=np.int64)
        for r in range(rows):
            a = np.flatnonzero(mask[par[r]] == 0)
            a = a[a != gr.EOS]
            tok[r] = gr.PAD if (r == 4 and s >= 20) else a[rng.integers(len(a))]
        ids[:, s + 1] = tok
        st.advance(torch.from_numpy(tok).to(dev), torch.from_numpy(par).to(dev))
        out["mask%d" % (s + 1)] = _sha(st.mask)
    out["active"] = _sha(st.active())
    out["replay"] = _sha(lib.grammar_replay(_grammar(), torch.from_numpy(ids).to(dev), V, carry=carry))
    return out


CASES = {
    "greedy-fp32-b3-lc250": (case_greedy, (F32, 3, 250, 12)),
    "greedy-bf16-b8-lc256": (case_greedy, (BF, 8, 256, 12)),
    "greedy-bf16-b9-lc256": (case_greedy, (BF, 9, 256, 12)),
    "greedy-bf16-b17-lc256": (case_greedy, (BF, 17, 256, 12)),
    "prefix3-bf16-b9": (case_greedy, (BF, 9, 256, 8, 3)),
    "ban-logp-bf16-b9": (case_ban_logp, ()),
    "sampled-logp-bf16-b9": (case_sampled, ()),
    "beam-3x4-ban-bf16": (case_beam, ()),
    "grammar-greedy-b9-beam-2x4": (case_grammar, ()),
    "grammar-alone-5rows": (case_grammar_alone, ()),
}


def run_case(name, dev):
    fn, args = CASES[name]
    out = fn(dev, *args)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_bits_equal_the_parent(dev, golden, name):
    assert run_case(name, dev) == golden["cases"][name]


def test_a_changed_norm_pointer_recaptures(dev):
    """A weights struct that differs from the last decode's in ln_ff[0] alone (a clone scaled by 2) forces a new capture,
    and the decode reads the new weight: its step logits are those of a fresh handle given that weight from the start.

    The parent commit FAILS this test, which is its point: its mrmt3_decoder_begin compared the six matrix pointers per
    layer but not ln_self / ln_cross / ln_ff, which the step graph bakes in as well, so it replayed the graph with the old
    norm weight (capture_count unchanged, the first decode's logits again)."""
    from mrmt3.decode import Decoder
    m, B, Lc, steps = _model(BF, dev, layers=1), 2, 256, 4
    enc = _enc(np.random.default_rng(307), m, B, Lc)
    scaled = (m.flat.master("decoder.block.0.layer.2.layer_norm.weight").detach() * 2).clone()

    def with_scaled_ln_ff(dec):
        plain = dec._weights

        def weights():
            w = plain()
            dec._wkeep[0]["ln_ff"][0] = scaled.data_ptr()        # the host array the struct's ln_ff points at
            return w

        dec._weights = weights

    def decode(dec):
        ckv = dec.cross_kv(enc, B, Lc)
        r, logits = _run(m, dec, ckv, B, Lc, steps)
        return logits.cpu()

    dec = Decoder(m, B, steps, Lc)
    first = decode(dec)
    assert dec.capture_count == 1
    with_scaled_ln_ff(dec)
    second = decode(dec)
    assert dec.graph_captured and dec.capture_count == 2
    fresh = Decoder(m, B, steps, Lc)
    with_scaled_ln_ff(fresh)
    want = decode(fresh)
    assert fresh.capture_count == 1
    assert torch.equal(second.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(second.view(torch.int32), first.view(torch.int32))       # the scaled weight reaches the logits
