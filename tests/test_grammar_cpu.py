"""The MT3 event grammar of constrained decoding on the host: tests/grammar_ref.py, the restatement the GPU
tests compare the kernel with, is itself checked here against the product's own event decoder and tokenizer.

  (1) sound: random walks over the allowed sets never get stuck and decode with 0 invalid and 0 dropped events;
  (2) complete for the data: every target row of the tokenizer fixtures is admitted token by token;
  (3) every rule of the table once, by hand;
  (4) the C ABI and the Python surface are there.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grammar_ref as gr  # noqa: E402
import test_tokenizer_cpu as tkfix  # noqa: E402  (the note-sequence fixtures of the tokenizer tests)
from contrib import vocabularies  # noqa: E402
from mrmt3.grammar import EventGrammar, resolve  # noqa: E402
from mrmt3.tokenizer import Tokenizer  # noqa: E402

SP = gr.SPECIAL


def _codec(bins=1):
    return vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=bins))


CODEC = _codec()
SHIFT, PITCH, VEL_OFF, VEL_ON, TIE, PROG, DRUM = 3, 1004, 1132, 1133, 1134, 1135, 1263


def test_id_layout_comes_from_the_codec():
    g = gr.GrammarRef(CODEC)
    assert g.rng == {"shift": (3, 1003), "pitch": (1004, 1131), "velocity": (1132, 1133), "tie": (1134, 1134),
                     "program": (1135, 1262), "drum": (1263, 1390)}
    assert g.V == 1491 and g.max_shift_steps == 204
    e = EventGrammar.from_codec(CODEC)
    assert (e.shift0, e.n_shift, e.pitch0, e.n_pitch, e.velocity0, e.n_velocity, e.tie, e.program0, e.n_program, e.drum0,
            e.n_drum, e.eos, e.pad, e.max_shift_steps, e.tie_section) == \
        (3, 1001, 1004, 128, 1132, 2, 1134, 1135, 128, 1263, 128, 1, 0, 204, True)
    assert EventGrammar.from_codec(CODEC, mel_length=512).max_shift_steps == 409
    assert EventGrammar.from_codec(CODEC, max_shift_steps=1000, tie_section=False).max_shift_steps == 1000
    e127 = EventGrammar.from_codec(_codec(127))
    assert (e127.velocity0, e127.n_velocity, e127.tie) == (1132, 128, 1260)
    assert resolve(False) is None and resolve(None) is None and resolve(True) == e and resolve(e127) is e127
    with pytest.raises(TypeError):
        resolve("yes")


def test_segment_limit_keeps_the_longest_shift():
    """max_shift_steps steps from a segment's start do not pass the next segment's start as inference computes it (the first
    frame time rounded down to the codec step).  `decode_events` compares the two in floating point: over the first 35
    segments (71 s) step 204 is kept at every boundary; later, 18 of 2000 boundaries lose that one last step to rounding
    (start + 2.04 > next start by one ulp), and one step fewer is kept everywhere."""
    sps, steps = CODEC.steps_per_second, gr.default_max_shift_steps(CODEC)
    starts = []
    for i in range(2000):
        t = i * 256 / 125.0
        starts.append(t - t % (1 / sps))
    pairs = list(zip(starts, starts[1:]))
    assert not any(a + steps / sps > b for a, b in pairs[:35])
    assert any(a + (steps + 1) / sps > b for a, b in pairs[:35])           # one more step is not kept
    assert not any(a + (steps - 1) / sps > b for a, b in pairs)


# ---- (1) -----------------------------------------------------------------------------------------------------------------
def test_random_walks_are_sound():
    rs = np.random.RandomState(0)
    body_tokens = 0
    for row in range(200):
        carry = gr.random_carry(rs) if row % 2 else None
        toks, g = gr.random_walk(CODEC, rs, 300, carry=carry)
        assert gr.count_invalid(toks, carry, CODEC) == (0, 0), (row, toks)
        body_tokens += g.mode == "body"
    assert body_tokens > 100            # most walks leave the tie section: the body rules are exercised


@pytest.mark.parametrize("bins,tie_section", [(127, True), (1, False), (127, False)])
def test_random_walks_other_codecs(bins, tie_section):
    codec, rs = _codec(bins), np.random.RandomState(bins + tie_section)
    for row in range(20):
        carry = gr.random_carry(rs) if row % 2 else None
        toks, _ = gr.random_walk(codec, rs, 300, carry=carry, tie_section=tie_section)
        assert gr.count_invalid(toks, carry, codec, tie_section=tie_section) == (0, 0), (row, toks)


# ---- (2) -----------------------------------------------------------------------------------------------------------------
def _fixture_rows(randomize):
    """Every row the tokenizer tests cut from their note-sequence fixtures, through `row_targets`."""
    tk = Tokenizer(is_randomize_tokens=randomize)
    rows = []
    for seed in (0, 1, 2):
        n_samples = int(12.0 * 16000) + 77
        feats = tk.tokenize(tkfix._random_notes(seed), n_samples)
        n_frames = len(feats["input_times"])
        rows += [(feats, s, 256) for s in (0, 256, 700, n_frames - 256)]
    for seed in (3, 4):
        feats = tk.tokenize(tkfix._random_notes(seed, n=40, dur=10.0, drums=False), int(11.0 * 16000))
        n_frames = len(feats["input_times"])
        rows += [(feats, s, min(256, n_frames - s)) for s in range(0, n_frames, 256)]
    feats = tk.tokenize(tkfix._random_notes(7, n=80, dur=6.0), int(6.5 * 16000))
    rows.append((feats, 0, 256))
    rng = np.random.RandomState(11)
    return tk, [tk.row_targets(f, s, n, rng=rng) for f, s, n in rows]


@pytest.mark.parametrize("randomize", [False, True])
def test_tokenizer_rows_are_admitted(randomize):
    tk, rows = _fixture_rows(randomize)
    assert len(rows) == 3 * 4 + 2 * 6 + 1
    n_tokens = 0
    for i, row in enumerate(rows):
        g = gr.GrammarRef(tk.codec, max_shift_steps=tk.codec.max_shift_steps)
        for j, tok in enumerate(row):
            assert g.allowed()[int(tok) + SP], (i, j, int(tok), row[:j + 1].tolist())
            g.push(int(tok) + SP)
        assert g.allowed()[gr.EOS], i
        n_tokens += len(row)
    assert n_tokens > 1000


# ---- (3) -----------------------------------------------------------------------------------------------------------------
def _after(tokens, **kw):
    g = gr.GrammarRef(CODEC, **kw)
    for t in tokens:
        assert g.allowed()[t], (t, tokens)
        g.push(t)
    return g


def test_rules_by_hand():
    a = _after([]).allowed()
    # start of the tie section: tie and programs only; no pitch before a program
    assert a[TIE] and a[PROG:PROG + 128].all() and a.sum() == 129
    assert not a[gr.EOS] and not a[gr.PAD] and not a[2] and not a[1391:].any()
    # a second declaration of the same pair in the tie section
    a = _after([PROG + 5, PITCH + 60]).allowed()
    assert not a[PITCH + 60] and a[PITCH + 61] and not a[VEL_ON] and not a[DRUM] and not a[SHIFT + 1]
    # with a carry only what was sounding may be declared
    a = _after([PROG + 5], carry={(5, 60), (6, 61)}).allowed()
    assert a[PITCH + 60] and not a[PITCH + 61] and a[PITCH:PITCH + 128].sum() == 1
    # after tie: the body.  Program carries over, velocity is still unset: no pitch, no drum
    g = _after([PROG + 5, PITCH + 60, TIE])
    a = g.allowed()
    assert g.active == {(5, 60)} and a[gr.EOS] and not a[TIE] and not a[PITCH:PITCH + 128].any() and not a[DRUM:DRUM + 128].any()
    # note-off of an inactive pitch; of the active one; then it is inactive
    a = _after([PROG + 5, PITCH + 60, TIE, VEL_OFF]).allowed()
    assert a[PITCH + 60] and a[PITCH:PITCH + 128].sum() == 1 and not a[DRUM:DRUM + 128].any()     # a drum under velocity off
    g = _after([PROG + 5, PITCH + 60, TIE, VEL_OFF, PITCH + 60])
    assert g.active == set() and not g.allowed()[PITCH:PITCH + 128].any()
    # the off of another program's note is inactive too
    assert not _after([PROG + 5, PITCH + 60, TIE, VEL_OFF, PROG + 6]).allowed()[PITCH + 60]
    # velocity on: any pitch (a re-onset is valid), drums
    g = _after([PROG + 5, PITCH + 60, TIE, VEL_ON, PITCH + 60, PITCH + 61])
    assert g.active == {(5, 60), (5, 61)} and g.allowed()[PITCH:PITCH + 128].all() and g.allowed()[DRUM:DRUM + 128].all()
    # a body row with no program: no pitch even under a velocity
    assert not _after([TIE, VEL_ON]).allowed()[PITCH:PITCH + 128].any() and _after([TIE, VEL_ON]).allowed()[DRUM]


def test_shift_boundaries():
    ms = 204
    a = _after([TIE]).allowed()                         # cur = acc = 0: shift 0 goes nowhere
    assert not a[SHIFT] and a[SHIFT + 1] and a[SHIFT + ms] and not a[SHIFT + ms + 1] and not a[SHIFT + 1000]
    g = _after([TIE, SHIFT + 50, VEL_ON])               # an event at step 50: cur = 50
    a = g.allowed()
    assert (g.cur, g.acc) == (50, 0)
    assert not a[SHIFT + 49] and not a[SHIFT + 50] and a[SHIFT + 51] and a[SHIFT + ms] and not a[SHIFT + ms + 1]
    g = _after([TIE, SHIFT + 50, VEL_ON, SHIFT + 51])   # inside a run every step moves on: acc = 51 > cur
    a = g.allowed()
    assert (g.cur, g.acc) == (50, 51)
    assert a[SHIFT + 1] and a[SHIFT + ms - 51] and not a[SHIFT + ms - 50]
    g = _after([TIE, SHIFT + ms, VEL_ON])               # at the end of the segment no shift is left
    assert not g.allowed()[SHIFT:SHIFT + 1001].any() and g.allowed()[gr.EOS]
    a = _after([TIE], max_shift_steps=1000).allowed()
    assert a[SHIFT + 1000] and not a[SHIFT]
    # what the rule is for: 204 steps are kept, 205 are dropped
    assert gr.count_invalid([TIE, SHIFT + ms, VEL_ON, DRUM + 40], None, CODEC) == (0, 0)
    assert gr.count_invalid([TIE, SHIFT + ms + 1, VEL_ON, DRUM + 40], None, CODEC)[1] > 0


def test_rejected_sequences_are_what_the_decoder_rejects():
    """One sequence per rule that the grammar refuses, and the product's decoder counting it invalid."""
    bad = [
        [TIE, PROG + 5, VEL_OFF, PITCH + 60],                     # note-off of an inactive pitch
        [PROG + 5, PITCH + 60, PITCH + 60, TIE],                  # declared twice
        [TIE, VEL_OFF, DRUM + 40],                                # drum under velocity off
        [TIE, TIE],                                               # tie outside the tie section
        [TIE, 1400],                                              # not an event
        [TIE, gr.PAD + 2],                                        # unk
    ]
    for seq in bad:
        g = gr.GrammarRef(CODEC)
        ok = True
        for t in seq:
            ok = ok and bool(g.allowed()[t])
            g.push(t)
        assert not ok, seq
        assert gr.count_invalid(seq, None, CODEC)[0] > 0, seq
    # a time shift that goes backwards
    g = _after([TIE, SHIFT + 50, VEL_ON])
    assert not g.allowed()[SHIFT + 40]
    assert gr.count_invalid([TIE, SHIFT + 50, VEL_ON, SHIFT + 40, DRUM + 40], None, CODEC)[0] > 0


def test_127_velocity_bins_and_no_tie_section():
    codec = _codec(127)
    g = gr.GrammarRef(codec, tie_section=False)
    lo_v, hi_v = (x + SP for x in codec.event_type_range("velocity"))
    prog, pitch = codec.event_type_range("program")[0] + SP, codec.event_type_range("pitch")[0] + SP
    tie = codec.event_type_range("tie")[0] + SP
    a = g.allowed()
    assert g.mode == "body" and a[gr.EOS] and not a[tie] and a[lo_v:hi_v + 1].all() and hi_v - lo_v == 127
    for t in (prog + 1, hi_v, pitch + 3):                  # the last velocity id is "on"
        assert g.allowed()[t]
        g.push(t)
    assert g.active == {(1, 3)}
    g.push(lo_v)                                           # the first is "off"
    a = g.allowed()
    assert a[pitch + 3] and a[pitch:pitch + 128].sum() == 1
    g.push(lo_v + 1)                                       # every other one is "on"
    assert g.allowed()[pitch:pitch + 128].all()
    # without a tie section the row starts with what was sounding
    g = gr.GrammarRef(codec, tie_section=False, carry={(1, 3)})
    for t in (prog + 1, lo_v):
        g.push(t)
    assert g.allowed()[pitch + 3]


def test_static_ban_and_the_tokens_that_may_not_be_banned():
    e = EventGrammar.from_codec(CODEC)
    e.check_ban(None)
    e.check_ban([PROG + 3, PITCH])
    with pytest.raises(ValueError):
        e.check_ban([gr.EOS])
    with pytest.raises(ValueError):
        e.check_ban([TIE])
    EventGrammar.from_codec(CODEC, tie_section=False).check_ban([TIE])
    a = gr.GrammarRef(CODEC, ban=[PROG + 3]).allowed()
    assert not a[PROG + 3] and a[PROG + 4] and a[TIE]


# ---- (4) -----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_keywords():
    import inspect
    from mrmt3 import decode, lib
    names = set(lib.header_symbols())
    want = {"mrmt3_decoder_set_grammar", "mrmt3_decoder_grammar_active", "mrmt3_grammar_advance", "mrmt3_grammar_state_bytes",
            "mrmt3_grammar_init", "mrmt3_grammar_active"}
    assert want <= names
    assert "typedef struct" in open(lib.HEADER_PATH).read() and "} mrmt3_grammar;" in open(lib.HEADER_PATH).read()
    assert lib.MIN_VERSION >= 120
    assert "grammar" in decode._Options.__dataclass_fields__ and decode._Options().grammar is None
    for fn in ("generate", "generate_2", "generate_beam", "generate_sample", "generate_best_of", "generate_songs"):
        assert inspect.signature(getattr(decode, fn)).parameters["constrained"].default is False, fn
    from mrmt3.module import MT3Module
    for fn in ("generate_beam", "generate_best_of", "generate_scored"):
        assert "constrained" in inspect.signature(getattr(MT3Module, fn)).parameters, fn
