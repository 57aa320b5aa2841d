"""Sampled decoding without a GPU: the host restatement `tests/sample_ref.py` against hand-worked rows and
against HF's warpers, the draw generator's statistics, the margins of the GPU test's seeds, and the Python surface
(`mrmt3.decode`, `MT3Module`, `InferenceHandler`) on stubs."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_ref as R  # noqa: E402


def _logits(probs):
    return np.log(np.asarray(probs, dtype=np.float64))[None, :].astype(np.float32)


def _kept(ref, row=0):
    return np.flatnonzero(ref.kept[row]).tolist()


# ---- the rule, by hand ---------------------------------------------------------------------------------------------
def test_top_k_keeps_ties_with_the_kth_value():
    lg = np.array([[3.0, 2.0, 2.0, 1.0, 0.0]], dtype=np.float32)
    ref = R.sample_ref(lg, top_k=2)
    assert _kept(ref) == [0, 1, 2]                                   # the 2nd largest value is 2.0: both 2.0s stay
    z = 1.0 + 2.0 * math.exp(-1.0)
    assert np.allclose(ref.hi[0], [1 / z, (1 + math.exp(-1)) / z, 1.0, 1.0, 1.0], atol=1e-15)
    assert np.allclose(ref.lo[0], [0.0, 1 / z, (1 + math.exp(-1)) / z, 1.0, 1.0], atol=1e-15)
    assert _kept(R.sample_ref(lg, top_k=1)) == [0] and _kept(R.sample_ref(lg, top_k=4)) == [0, 1, 2, 3]
    assert _kept(R.sample_ref(lg, top_k=5)) == _kept(R.sample_ref(lg, top_k=9)) == _kept(R.sample_ref(lg)) == [0, 1, 2, 3, 4]


def test_top_p_always_keeps_the_most_likely_token():
    lg = _logits([0.2, 0.7, 0.1])
    assert _kept(R.sample_ref(lg, top_p=0.5)) == [1]                 # 0.7 alone exceeds top_p: it stays, alone
    assert _kept(R.sample_ref(lg, top_p=1e-6)) == [1]
    assert _kept(R.sample_ref(lg, top_p=0.75)) == [0, 1]             # mass above token 0 is 0.7 <= 0.75; above token 2 is 0.9
    assert _kept(R.sample_ref(lg, top_p=0.95)) == [0, 1, 2]
    ref = R.sample_ref(lg, top_p=0.75)
    assert np.allclose(ref.hi[0], [0.2 / 0.9, 1.0, 1.0], atol=1e-7)  # renormalised over the kept set, ascending index


def test_top_p_keeps_or_cuts_a_tie_group_whole():
    lg = _logits([0.1, 0.2, 0.5, 0.2])                               # tokens 1 and 3 are equal: mass above them is 0.5
    assert lg[0, 1] == lg[0, 3]
    assert _kept(R.sample_ref(lg, top_p=0.6)) == [1, 2, 3]           # HF would cut between the twins (0.5 + 0.2 > 0.6)
    assert _kept(R.sample_ref(lg, top_p=0.55)) == [1, 2, 3]          # the cut at the group's leading edge: both stay
    assert _kept(R.sample_ref(lg, top_p=0.45)) == [2]                # ... just ahead of it: both go
    assert _kept(R.sample_ref(lg, top_p=0.89)) == [1, 2, 3]          # at the group's trailing edge token 0 (0.9 above) goes
    assert _kept(R.sample_ref(lg, top_p=0.91)) == [0, 1, 2, 3]


def test_ban_and_temperature():
    lg = np.array([[2.0, 1.0, 0.0, 5.0]], dtype=np.float32)
    ref = R.sample_ref(lg, ban=[3], temperature=2.0)
    assert _kept(ref) == [0, 1, 2]
    e = np.exp(np.array([1.0, 0.5, 0.0]) - 1.0)
    assert np.allclose(ref.hi[0, :3], np.cumsum(e) / e.sum(), atol=1e-15) and ref.hi[0, 3] == ref.lo[0, 3]
    mask = np.array([0, 0, 0, 1], dtype=np.uint8)
    assert np.array_equal(R.sample_ref(lg, ban=mask, temperature=2.0).hi, ref.hi)
    cold = R.sample_ref(lg, ban=[3], temperature=0.5)                 # T < 1 sharpens
    assert cold.hi[0, 0] > ref.hi[0, 0]
    assert _kept(R.sample_ref(lg, ban=[3], top_k=1)) == [0]          # the ban comes first: top-1 of the rest
    # pick / check agree with the intervals
    u = np.array([0.0]), np.array([ref.hi[0, 0]]), np.array([0.999999])
    assert [int(ref.pick(x)[0]) for x in u] == [0, 1, 2]
    wrong, slack = ref.check(np.array([0]), np.array([ref.hi[0, 0] + 1e-5]))
    assert not wrong[0] and slack[0]
    wrong, _ = ref.check(np.array([3]), np.array([0.5]))
    assert wrong[0]


def test_rows_that_are_not_drawn_from():
    lg = np.array([[0.0, np.nan, 1.0, np.nan], [-np.inf] * 4, [0.0, 1.0, 2.0, 3.0], [0.0, np.inf, 1.0, np.inf]], dtype=np.float32)
    ref = R.sample_ref(lg, top_p=0.9)
    assert ref.greedy.tolist() == [True, True, False, True] and ref.greedy_token.tolist() == [1, 0, 3, 1]
    assert R.sample_ref(lg, ban=[1, 3]).greedy.tolist() == [False, True, False, False]      # the NaNs are banned away
    assert R.sample_ref(lg[2:3], ban=[0, 1, 2, 3]).greedy.tolist() == [True]                # all banned: token 0
    assert ref.pick(np.full(4, 0.5))[[0, 1, 3]].tolist() == [1, 0, 1]


def test_kept_set_equals_hf_warpers_on_rows_of_distinct_logits():
    g = np.random.default_rng(7)
    n = 0
    for T, k, p in [(1.0, 0, 1.0), (1.0, 7, 1.0), (1.0, 0, 0.9), (0.5, 7, 0.3), (2.0, 50, 0.9), (0.7, 3, 0.5), (1.3, 0, 0.3),
                    (1.0, 1, 0.9), (2.0, 0, 0.999), (0.5, 0, 1e-6)]:
        lg = (2.0 * g.standard_normal((100, 50))).astype(np.float32)
        assert all(len(np.unique(r)) == 50 for r in lg)
        assert np.array_equal(R.sample_ref(lg, None, T, k, p).kept, R.hf_kept(lg, T, k, p)), (T, k, p)
        n += len(lg)
    assert n == 1000


# ---- the generator -------------------------------------------------------------------------------------------------
GEN_SEED = 20240

def _pairs():
    r, t = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return r.reshape(-1), t.reshape(-1)


def test_u_is_uniform_over_rows_and_steps():
    r, t = _pairs()
    u = R.uniform(GEN_SEED, r, t)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u * (1 << 24), np.floor(u * (1 << 24)))
    n = np.bincount((u * 16).astype(int), minlength=16)
    chi = float(((n - 4096.0) ** 2 / 4096.0).sum())
    print(f"[u] 16 bins over 65536 (row, step) pairs: chi-square {chi:.2f}")
    assert chi < 37.70                                               # 0.999 quantile, 15 degrees of freedom
    # along one row (steps) and along one step (rows) alike: neither index alone drives the stream
    for a, b in ((np.zeros(4096, int), np.arange(4096)), (np.arange(4096), np.zeros(4096, int))):
        n = np.bincount((R.uniform(GEN_SEED, a, b) * 16).astype(int), minlength=16)
        assert float(((n - 256.0) ** 2 / 256.0).sum()) < 37.70


def test_draws_follow_an_8_token_distribution():
    r, t = _pairs()
    lg = R.case_logits("live8", 64, 1, "live8")
    ref = R.sample_ref(lg)
    cols = np.flatnonzero(ref.kept[0])
    prob = (ref.hi - ref.lo)[0, cols]
    assert len(cols) == 8 and abs(prob.sum() - 1.0) < 1e-12
    u = R.uniform(GEN_SEED, r, t)
    big = R.Rows(*(np.repeat(x, len(u), 0) for x in (ref.kept, ref.lo, ref.hi, ref.greedy, ref.greedy_token)))
    tok = big.pick(u)
    assert np.isin(tok, cols).all()
    n = np.array([(tok == c).sum() for c in cols])
    chi = float(((n - 65536 * prob) ** 2 / (65536 * prob)).sum())
    print(f"[draw] 8 tokens, probabilities {np.round(prob, 4).tolist()}: chi-square {chi:.2f}")
    assert chi < 24.32                                               # 0.999 quantile, 7 degrees of freedom
    wrong, slack = big.check(tok, u)
    assert not wrong.any() and not slack.any()


def test_two_seeds_give_different_streams():
    r, t = _pairs()
    a, b = R.u24(GEN_SEED, r, t), R.u24(GEN_SEED + 1, r, t)
    assert (a != b).mean() > 0.99
    assert (R.u24(GEN_SEED, r, t) == a).all()                        # a pure function
    assert (R.u24(GEN_SEED + (1 << 32), r, t) != a).mean() > 0.99    # the high half of a 64-bit seed counts
    assert (R.u24(GEN_SEED, r + 1, t) != a).mean() > 0.99 and (R.u24(GEN_SEED, r, t + 1) != a).mean() > 0.99


def test_no_draw_of_a_kernel_case_sits_on_an_interval_edge():
    """The seeds of `sample_ref.CASES` keep every u further than SLACK from every interval edge of its row, so the kernel
    test may ask for the host's token, not just for a token within the slack."""
    seen = set()
    for name, V, rows, kind, ban, T, k, p, seed in R.CASES:
        ref = R.sample_ref(R.case_logits(name, V, rows, kind), ban, T, k, p)
        u = R.uniform(seed, R.CASE_ROW0 + np.arange(rows), R.CASE_STEP)
        assert float(ref.edge_distance(u).min()) > R.SLACK, name
        wrong, slack = ref.check(ref.pick(u), u)
        assert not wrong.any() and not slack.any(), name
        seen |= {("V", V), ("rows", rows), ("T", T), ("k", k), ("p", p), ("ban", ban is not None), kind}
    want = {("V", v) for v in (5, 64, 65, 1536, 2048)} | {("rows", r) for r in (1, 8, 9, 4096)} | \
        {("T", x) for x in (0.5, 1.0, 2.0)} | {("k", x) for x in (0, 1, 7)} | {("p", x) for x in (1.0, 0.9, 0.3)} | \
        {("ban", True), "gauss", "ties", "live8"}
    assert want <= seen, want - seen


# ---- the Python surface on stubs -----------------------------------------------------------------------------------
def test_sampling_argument_ranges():
    from mrmt3.decode import Sampling, _sampling
    assert _sampling(False, -1.0, -3, 7.0, -1) is None               # do_sample=False looks at nothing
    sp = _sampling(True, 0.7, 5, 0.9, 11)
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.7, 5, 0.9, 11) and sp.shifted(3).seed == 14
    assert sp.shifted(3).top_k == 5 and Sampling(seed=2 ** 64 - 1).shifted(2).seed == 1
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(seed=-1),
                dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            Sampling(**bad)


class _StubModel:
    """What the argument checks of `mrmt3.decode` look at before any tensor is touched."""
    engine = None
    cfg = {"vocab_size": 1536, "eos_token_id": 1}

    def __init__(self, variant):
        self.VARIANT = variant


def test_decode_entry_points_refuse_what_sampling_cannot_do():
    from mrmt3 import decode
    x = torch.zeros(2, 4, 512)
    for variant in ("t5", "segmem_v2"):
        with pytest.raises(ValueError, match="beam search does not sample"):
            decode.generate_beam(_StubModel(variant), x, num_beams=2, do_sample=True)
    with pytest.raises(ValueError, match="beam search does not sample"):
        decode.generate_songs(_StubModel("segmem_v2"), [x], num_beams=2, do_sample=True)
    for variant in ("segmem_v2", "segmem_v2_with_prev"):
        with pytest.raises(ValueError, match="one sample per segment"):
            decode.generate_sample(_StubModel(variant), x, num_return_sequences=2)
        with pytest.raises(ValueError, match="plain T5"):
            decode.generate_best_of(_StubModel(variant), x, 2)
    with pytest.raises(ValueError):
        decode.generate_sample(_StubModel("t5"), x, num_return_sequences=0)
    with pytest.raises(ValueError):
        decode.generate_sample(_StubModel("t5"), x, temperature=0.0)
    with pytest.raises(ValueError):
        decode.generate(_StubModel("t5"), x, do_sample=True, top_p=0.0)
    with pytest.raises(ValueError):
        decode.generate_2(_StubModel("segmem_v1"), x, do_sample=True, top_k=-2)
    with pytest.raises(ValueError):
        decode.generate_best_of(_StubModel("t5"), x, 0)
    with pytest.raises(RuntimeError, match="device tensors"):       # valid arguments reach the device check: no CPU path
        decode.generate_sample(_StubModel("t5"), x, num_return_sequences=2)


def test_module_surface_has_the_sampling_calls():
    import inspect
    from mrmt3.module import MT3Module
    sig = inspect.signature(MT3Module.generate_sample)
    assert list(sig.parameters)[1:] == ["inputs", "max_length", "temperature", "top_k", "top_p", "seed", "num_return_sequences",
                                        "bad_token_ids", "return_logprobs"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [1024, 1.0, 0, 1.0, 0, 1, None, False]
    assert list(inspect.signature(MT3Module.generate_best_of).parameters)[1:3] == ["inputs", "n"]
    from mrmt3 import decode
    for fn in (decode.generate, decode.generate_2, decode.generate_songs, decode.generate_beam):
        prm = inspect.signature(fn).parameters
        assert [(k, prm[k].default) for k in ("do_sample", "temperature", "top_k", "top_p", "seed")] == \
            [("do_sample", False), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("seed", 0)], fn.__name__
    assert "sampling" in inspect.signature(decode.Decoder.run).parameters
    from mrmt3 import lib
    assert {"mrmt3_decoder_set_sampling", "mrmt3_sample_logits"} <= set(lib._SIGS) and hasattr(lib, "sample_logits")
    import ctypes as C
    assert lib._SIGS["mrmt3_decoder_set_sampling"] == (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_ulonglong, C.c_void_p])
    assert len(lib._SIGS["mrmt3_sample_logits"][1]) == 13


def test_best_of_select_on_hand_made_rows():
    from mrmt3.decode import best_of_select
    eos = 1
    ids = torch.tensor([[0, 5, 6, 1, 0, 0],        # group 0: -0.6 up to its EOS (what follows must not count)
                        [0, 5, 1, 0, 0, 0],        #          -0.5: the best
                        [0, 7, 8, 9, 9, 9],        #          no EOS: the whole row, -2.5
                        [0, 4, 1, 0, 0, 0],        # group 1: -1.0
                        [0, 3, 3, 1, 0, 0],        #          -1.0: a tie, the lowest j wins
                        [0, 2, 2, 2, 2, 2]])       #          no EOS, -1.0 as well
    lp = torch.tensor([[0.0, -0.2, -0.2, -0.2, -9.0, -9.0],
                       [0.0, -0.25, -0.25, 5.0, 5.0, 0.0],
                       [0.0, -0.5, -0.5, -0.5, -0.5, -0.5],
                       [0.0, -0.5, -0.5, 0.0, 0.0, 0.0],
                       [0.0, -0.25, -0.25, -0.5, 0.0, 0.0],
                       [0.0, -0.2, -0.2, -0.2, -0.2, -0.2]])
    out, out_lp, j = best_of_select(ids, lp, 3, eos)
    assert j.tolist() == [1, 0] and torch.equal(out, ids[[1, 3]]) and torch.equal(out_lp, lp[[1, 3]])
    _, _, j = best_of_select(ids, lp, 1, eos)
    assert j.tolist() == [0] * 6
    _, _, j = best_of_select(ids, lp, 6, eos)
    assert j.tolist() == [1]
    lp2 = lp.clone()
    lp2[5, 5] = 0.1                                 # the EOS-less row now sums to -0.7: it wins group 1
    assert best_of_select(ids, lp2, 3, eos)[2].tolist() == [1, 2]
    with pytest.raises(ValueError):
        best_of_select(ids, lp, 4, eos)


class _Recorder:
    """Stands for a model behind `InferenceHandler`: records every decode call, returns EOS-only rows."""
    VARIANT = "t5"
    config = type("Cfg", (), {"eos_token_id": 1})()

    def __init__(self):
        self.calls = []

    def to(self, device):
        return self

    def _out(self, inputs, scored):
        ids = torch.zeros(inputs.shape[0], 3, dtype=torch.int64)
        ids[:, 1] = 1
        return (ids, torch.zeros(ids.shape)) if scored else ids

    def generate(self, inputs, max_length=1024, **kw):
        self.calls.append(("generate", kw))
        return self._out(inputs, False)

    def generate_beam(self, inputs, **kw):
        self.calls.append(("generate_beam", kw))
        return self._out(inputs, kw.get("return_logprobs", False))

    def generate_scored(self, inputs, **kw):
        self.calls.append(("generate_scored", kw))
        return self._out(inputs, True)

    def generate_sample(self, inputs, **kw):
        self.calls.append(("generate_sample", kw))
        return self._out(inputs, kw.get("return_logprobs", False))

    def generate_best_of(self, inputs, n, **kw):
        self.calls.append(("generate_best_of", dict(kw, n=n)))
        return self._out(inputs, True)


def _handler(monkeypatch, model, decode_options, n_seg=12):
    import inference
    h = inference.InferenceHandler(model=model, device=torch.device("cpu"), decode_options=decode_options)
    monkeypatch.setattr(h, "_preprocess", lambda audio: (torch.zeros(n_seg, 4, 512), np.zeros((n_seg, 256))))
    return h


def test_inference_handler_gives_every_batch_its_own_seed(monkeypatch):
    m = _Recorder()
    h = _handler(monkeypatch, m, True)
    h.inference(None, batch_size=5, max_length=8, return_tokens=True, do_sample=True, temperature=0.8, top_k=4, top_p=0.9, seed=100,
                valid_programs=[0])
    assert [c[0] for c in m.calls] == ["generate_sample"] * 3
    assert [c[1]["seed"] for c in m.calls] == [100, 101, 102]
    for _, kw in m.calls:
        assert (kw["temperature"], kw["top_k"], kw["top_p"], kw["return_logprobs"]) == (0.8, 4, 0.9, False)
        assert kw["bad_token_ids"] and kw["max_length"] == 8
    m.calls.clear()
    h.inference(None, batch_size=5, max_length=8, return_tokens=True, do_sample=True, seed=7, with_confidence=True)
    assert [(c[0], c[1]["seed"], c[1]["return_logprobs"]) for c in m.calls] == [("generate_sample", 7 + i, True) for i in range(3)]
    m.calls.clear()
    h.inference(None, batch_size=6, max_length=8, return_tokens=True, best_of=4, seed=50)       # best_of implies sampling
    assert [(c[0], c[1]["n"], c[1]["seed"]) for c in m.calls] == [("generate_best_of", 4, 50), ("generate_best_of", 4, 51)]
    m.calls.clear()
    h.inference_many([None, None], max_length=8, return_tokens=True, do_sample=True, seed=9)
    assert [(c[0], c[1]["seed"]) for c in m.calls] == [("generate_sample", 9)]
    with pytest.raises(ValueError, match="beam search does not sample"):
        h.inference(None, max_length=8, do_sample=True, num_beams=2)
    with pytest.raises(ValueError):
        h.inference(None, max_length=8, best_of=0)


def test_inference_handler_ignores_sampling_without_decode_options(monkeypatch):
    m = _Recorder()
    h = _handler(monkeypatch, m, False)
    h.inference(None, batch_size=5, max_length=8, return_tokens=True, do_sample=True, temperature=0.8, seed=100, best_of=3)
    assert [c[0] for c in m.calls] == ["generate"] * 3 and all(c[1] == {} for c in m.calls)
    m.calls.clear()
    h.inference(None, batch_size=12, max_length=8, return_tokens=True, do_sample=True, with_confidence=True)
    assert [c[0] for c in m.calls] == ["generate_scored"] and "seed" not in m.calls[0][1]


def test_best_of_is_refused_for_the_memory_models(monkeypatch):
    m = _Recorder()
    m.VARIANT = "segmem_v2_with_prev"
    m.generate_songs = lambda songs, **kw: [torch.zeros(s.shape[0], 8, dtype=torch.int64) for s in songs]
    h = _handler(monkeypatch, m, True)
    with pytest.raises(ValueError, match="plain T5"):
        h.inference(None, max_length=8, best_of=2)
    with pytest.raises(ValueError, match="plain T5"):
        h.inference_many([None], max_length=8, best_of=2)
    seen = {}
    m.generate_songs = lambda songs, **kw: seen.update(kw) or [torch.zeros(s.shape[0], 8, dtype=torch.int64) for s in songs]
    h.inference_many([None], max_length=8, return_tokens=True, do_sample=True, top_k=3, seed=21)
    assert seen["do_sample"] is True and seen["seed"] == 21 and seen["top_k"] == 3
