"""Beam search and program bans, host side: the ban list of the reference's `_get_program_ids`, the inference handler's
dispatch under decode_options, the float64 scorer restatement (tests/beam_ref.py) on hand-derived cases, and the C ABI
declarations of the new entry points."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from beam_ref import BeamRef  # noqa: E402

PROGRAM_LO = 1132        # codec.event_type_range('program') = (1132, 1259); ids are offset by the 3 special tokens


def test_program_ban_ids_exact():
    from inference import program_ban_ids
    everything = program_ban_ids(range(128))
    assert everything == []
    none_valid = program_ban_ids([])
    assert none_valid == list(range(1135, 1262))             # p in range(127): program 127 (id 1262) is never banned
    assert 1262 not in none_valid and len(none_valid) == 127
    assert program_ban_ids([0]) == list(range(1136, 1262))
    assert program_ban_ids([0, 32, 127]) == [PROGRAM_LO + 3 + p for p in range(127) if p not in (0, 32)]
    assert program_ban_ids({5, 6}) == [PROGRAM_LO + 3 + p for p in range(127) if p not in (5, 6)]


class _StubModel:
    """Records the decode calls the handler makes."""

    def __init__(self, songs=False):
        self.calls = []
        self.config = type("C", (), {"eos_token_id": 1})()
        if songs:
            self.generate_songs = self._generate_songs

    def to(self, device):
        return self

    def _ids(self, n):
        return torch.tensor([[0, 5, 6, 1]] * n, dtype=torch.int64)

    def generate(self, inputs, max_length=1024, **kw):
        self.calls.append(("generate", dict(max_length=max_length, **kw)))
        return self._ids(inputs.shape[0])

    def generate_beam(self, inputs, num_beams=1, max_length=1024, length_penalty=1.0, bad_token_ids=None, poll_every=64):
        self.calls.append(("generate_beam", dict(num_beams=num_beams, max_length=max_length,
                                                 length_penalty=length_penalty, bad_token_ids=bad_token_ids)))
        return self._ids(inputs.shape[0])

    def _generate_songs(self, songs, max_length=1024, **kw):
        self.calls.append(("generate_songs", dict(max_length=max_length, **kw)))
        return [self._ids(x.shape[0]) for x in songs]


def _handler(model, monkeypatch, decode_options=None, env=None):
    from inference import InferenceHandler
    if env is None:
        monkeypatch.delenv("MRMT3_DECODE_OPTIONS", raising=False)
    else:
        monkeypatch.setenv("MRMT3_DECODE_OPTIONS", env)
    h = InferenceHandler(model=model, device=torch.device("cpu"), decode_options=decode_options)
    # 7 segments of (fake) log-mel frames: no spectrogram kernel needed for the dispatch under test
    h._preprocess = lambda audio: (torch.zeros(7, 4, 8), np.zeros((7, 4)))
    return h


def test_handler_knob_off_calls_generate_as_today(monkeypatch):
    m = _StubModel()
    h = _handler(m, monkeypatch)
    assert h.decode_options is False
    h.inference(np.zeros(16), valid_programs=[0, 1], num_beams=4, batch_size=5, max_length=32, return_tokens=True)
    assert m.calls == [("generate", dict(max_length=32))] * 2


def test_handler_knob_on_calls_generate_beam_with_the_reference_keywords(monkeypatch):
    from inference import program_ban_ids
    for kw in (dict(env="1"), dict(decode_options=True, env="0")):
        m = _StubModel()
        h = _handler(m, monkeypatch, **kw)
        assert h.decode_options is True
        res, _ = h.inference(np.zeros(16), valid_programs=[0, 33], num_beams=4, batch_size=5, max_length=32,
                             return_tokens=True)
        want = dict(num_beams=4, max_length=32, length_penalty=0.4, bad_token_ids=program_ban_ids([0, 33]))
        assert m.calls == [("generate_beam", want)] * 2
        assert res[0].shape == (5, 3)
    m = _StubModel()
    h = _handler(m, monkeypatch, env="1")
    h.inference(np.zeros(16), return_tokens=True, max_length=16)
    assert m.calls[0] == ("generate_beam", dict(num_beams=1, max_length=16, length_penalty=0.4, bad_token_ids=None))


def test_handler_get_program_ids_has_the_reference_shape(monkeypatch):
    from inference import program_ban_ids
    h = _handler(_StubModel(), monkeypatch)
    assert h._get_program_ids([3]) == [[i] for i in program_ban_ids([3])]


def test_inference_many_honours_programs_and_beams(monkeypatch):
    from inference import program_ban_ids
    m = _StubModel(songs=True)
    h = _handler(m, monkeypatch)
    h.inference_many([np.zeros(16), np.zeros(16)], max_length=8, return_tokens=True)
    assert m.calls == [("generate_songs", dict(max_length=8))]
    m.calls.clear()
    h.inference_many([np.zeros(16)], max_length=8, return_tokens=True, valid_programs=[1], num_beams=3)
    assert m.calls == [("generate_songs", dict(max_length=8, num_beams=3, length_penalty=0.4,
                                               bad_token_ids=program_ban_ids([1])))]
    m = _StubModel()
    h = _handler(m, monkeypatch)
    out = h.inference_many([np.zeros(16), np.zeros(16)], max_length=8, return_tokens=True, num_beams=2)
    assert m.calls == [("generate_beam", dict(num_beams=2, max_length=8, length_penalty=0.4, bad_token_ids=None))]
    assert len(out) == 2


# ---- the scorer restatement on hand-derived cases (V = 5: pad 0, EOS 1, tokens 2..4; k = 2) ------------------------

def _lg(*rows):
    """Logits whose log-softmax is log(p) exactly (each row of probabilities sums to 1)."""
    a = np.log(np.asarray(rows, dtype=np.float64))
    assert np.allclose(np.exp(a).sum(-1), 1.0)
    return a


def _same(hyps, want):
    return len(hyps) == len(want) and all(abs(a[0] - b[0]) < 1e-12 and a[1:] == b[1:] for a, b in zip(hyps, want))


def test_scorer_skips_an_eos_ranked_at_or_below_k():
    ref = BeamRef(1, 2, 5, length_penalty=1.0)
    p, tk, sc = ref.step(0, _lg([0.01, 0.45, 0.27, 0.26, 0.01], [0.2] * 5))
    # beam 1 starts at -1e9: the top 4 are beam 0's; EOS (rank 0) is a hypothesis of length 1
    assert list(p) == [0, 0] and list(tk) == [2, 3]
    assert _same(ref.hyps[0], [(math.log(0.45), 0, 0)])
    np.testing.assert_allclose(sc, [math.log(0.27), math.log(0.26)], rtol=1e-12)
    # step 1: ranks (0,EOS) .27*.5, (0,2) .27*.3, (1,EOS) .26*.3, (0,3) .27*.1 -> the rank-2 EOS is skipped
    ref2 = BeamRef(1, 2, 5, length_penalty=1.0)
    ref2.scores = np.log([0.5, 0.2])
    p, tk, sc = ref2.step(1, _lg([0.02, 0.5, 0.3, 0.1, 0.08], [0.05, 0.6, 0.15, 0.1, 0.1]))
    assert list(p) == [0, 0] and list(tk) == [2, 3]
    assert _same(ref2.hyps[0], [(math.log(0.5 * 0.5) / 2, 1, 0)])      # only beam 0's EOS (rank 0)
    np.testing.assert_allclose(sc, np.log([0.5 * 0.3, 0.5 * 0.1]), rtol=1e-12)
    assert not ref2.done[0]


def test_scorer_done_test_with_length_penalty():
    """Two hypotheses held, worst -1.5; best candidate at step 2 (cur_len 3) scores -3: done iff
    -1.5 >= -3 / 3**lp, true for lp = 0.4 (-1.933) and false for lp = 1 (-1)."""
    for lp, want in ((0.4, True), (1.0, False)):
        ref = BeamRef(1, 2, 5, length_penalty=lp)
        ref.hyps[0] = [(-1.2, 1, 0), (-1.5, 2, 1)]
        ref.worst[0] = -1.5
        ref.scores = np.array([-2.0, -2.5])
        p, tk, _ = ref.step(2, _lg([0.1, 0.1, math.exp(-1), 0.6 - math.exp(-1), 0.2], [0.2] * 5))
        assert list(tk) == [2, 3] and list(p) == [0, 0]
        assert len(ref.hyps[0]) == 2                 # no EOS in the top 4
        assert bool(ref.done[0]) == want, (lp, ref.done[0])
        assert ref.done_margins[-1] == pytest.approx(abs(-1.5 + 3 / 3 ** lp))
    # a done group emits pad, keeps its rows and scores 0
    ref = BeamRef(1, 2, 5, length_penalty=0.4)
    ref.done[0] = True
    p, tk, sc = ref.step(3, _lg([0.2] * 5, [0.2] * 5))
    assert list(p) == [0, 1] and list(tk) == [0, 0] and list(sc) == [0, 0]


def _two_steps(lp=1.0):
    ref = BeamRef(1, 2, 5, length_penalty=lp)
    ref.step(0, _lg([0.05, 0.05, 0.5, 0.3, 0.1], [0.2] * 5))
    p, tk, _ = ref.step(1, _lg([0.02, 0.02, 0.06, 0.6, 0.3], [0.02, 0.02, 0.9, 0.03, 0.03]))
    assert list(p) == [0, 1] and list(tk) == [3, 2]      # (0,3) .30 > (1,2) .27 > (0,4) .15
    return ref


def test_finalize_adds_running_beams_and_writes_eos_only_below_the_limit():
    ref = _two_steps()
    out, best = ref.finalize(2, max_length=2)           # length 3 = 1 + max_length: no EOS, width 3
    assert out.tolist() == [[0, 2, 3]]
    assert _same(best[:1], [(math.log(0.3) / 3, 2, 0)])
    assert [e[2] for e in ref.hyps[0]] == [0, 1]        # both running beams became hypotheses
    ref = _two_steps()
    out, _ = ref.finalize(2, max_length=4)              # shorter than 1 + max_length: EOS, width min(3 + 1, 5)
    assert out.tolist() == [[0, 2, 3, 1]]


def test_finalize_pads_groups_of_different_lengths_and_takes_the_last_of_equal_best():
    ref = BeamRef(2, 2, 5, length_penalty=1.0)
    ref.bp = [(np.array([0, 0, 2, 2]), np.array([2, 3, 4, 2]))]
    ref.hyps = [[(-1.0, 0, 0), (-1.0, 1, 1)], [(-0.5, 1, 2), (-2.0, 0, 3)]]
    ref.done = [True, True]
    out, best = ref.finalize(1, max_length=6)
    assert best[0] == (-1.0, 1, 1)                      # equal best scores: the one added last
    assert out.tolist() == [[0, 3, 1], [0, 4, 1]]


def test_beam_abi_is_declared_and_bound():
    from mrmt3 import lib
    names = set(lib.header_symbols())
    for n in ("mrmt3_decoder_set_ban", "mrmt3_decoder_begin_beam", "mrmt3_decoder_beam_finalize"):
        assert n in names and n in lib._SIGS, n
    assert len(lib._SIGS["mrmt3_decoder_begin_beam"][1]) == 16


def test_beam_arguments_are_checked_before_any_device_work():
    from mrmt3 import decode
    x = torch.zeros(1, 4, 512)
    with pytest.raises(ValueError):
        decode.generate_beam(object(), x, num_beams=9)
    with pytest.raises(ValueError):
        decode.generate_beam(object(), x, num_beams=0)
    with pytest.raises(ValueError):
        decode.generate_2(object(), x, num_beams=2)
    with pytest.raises(ValueError):
        decode.generate_songs(object(), [x], num_beams=9)
