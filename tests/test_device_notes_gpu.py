"""Token rows -> notes on a real MI355X: mrmt3_notes_decode_fwd against the contract's host restatement
(`mrmt3.notes.decode_notes_host`, which tests/test_device_notes_cpu.py holds to the definition) over the corpus and the
hand-written cases of tests/_notes.py, unscored and scored, then `decode_notes` and the inference handler on top of it.
Every comparison is equality: integers, f64 times and f32 scores bit for bit."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _notes as N  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                                       # 32-bit words on either side of every output array
SENTINEL = -0x5a5a5a5a


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    return N.corpus() + N.hand_cases()


def _fit(case, ld):
    """The case at row length `ld`: columns cut (a row may lose its EOS, and with it its tokens) or padded with PAD."""
    rows = len(case.ids)
    ids = np.full((rows, ld), N.PAD, np.int64)
    logp = np.zeros((rows, ld), np.float32)
    w = min(ld, case.ids.shape[1])
    ids[:, :w], logp[:, :w] = case.ids[:, :w], case.logp[:, :w]
    return dataclasses.replace(case, ids=ids, logp=logp, expect=None)


def _guarded(words, dev):
    return torch.full((words + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int32)


def _inner(buf, dtype):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "a guard word was written"
    return host[GUARD:-GUARD].view(dtype)


def _launch(batch, scored, dev, grammar=None, expect_rc=0, **over):
    """One launch through the C ABI for the recordings `batch` (cases of one row length), guard words around every output:
    a list of NoteArrays, one per recording, with the kernel's status."""
    from mrmt3 import lib, notes
    ld = batch[0].ids.shape[1]
    assert all(c.ids.shape[1] == ld for c in batch)
    ids = np.concatenate([c.ids for c in batch])
    rows, n_rec = len(ids), len(batch)
    seg_first = np.cumsum([0] + [len(c.ids) for c in batch]).astype(np.int32)
    start = np.concatenate([c.start for c in batch])
    limit = np.concatenate([N.limits(c.start) for c in batch])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(ids=up(ids), logp=up(np.concatenate([c.logp for c in batch])) if scored else None, seg_first=up(seg_first),
             start=up(start), limit=up(limit), vel=up(notes.velocity_table(N.CODEC)))
    cap = rows * (ld - 1)
    out = {k: _guarded(n_rec, dev) for k in ("n_notes", "invalid", "dropped", "status")}
    out.update(total=_guarded(2 * n_rec, dev), times=_guarded(4 * cap, dev), meta=_guarded(4 * cap, dev),
               logc=_guarded(cap, dev) if scored else None)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    po = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
    g = (grammar or N.grammar()).c_struct()
    args = dict(g=ctypes.byref(g), ids=p(d["ids"]), logp=p(d["logp"]), rows=rows, ld=ld, seg_first=p(d["seg_first"]), n_rec=n_rec,
                start=p(d["start"]), limit=p(d["limit"]), vel=p(d["vel"]), n_notes=po(out["n_notes"]), invalid=po(out["invalid"]),
                dropped=po(out["dropped"]), status=po(out["status"]), total=po(out["total"]), times=po(out["times"]),
                meta=po(out["meta"]), logc=po(out["logc"]), stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    args.update(over)
    rc = lib.load().mrmt3_notes_decode_fwd(*args.values())
    assert rc == expect_rc, (rc, lib.load().mrmt3_last_error())
    torch.cuda.synchronize()
    host = {k: _inner(v, np.int32) for k, v in out.items() if k in ("n_notes", "invalid", "dropped", "status", "meta")}
    host["total"], host["times"] = _inner(out["total"], np.float64), _inner(out["times"], np.float64)
    host["logc"] = _inner(out["logc"], np.float32) if scored else None
    if rc != 0:
        for k, v in host.items():
            assert v is None or (v.view(np.int32) == SENTINEL).all(), "an output was written by a refused call"
        return None
    result = []
    for r in range(n_rec):
        a, n = int(seg_first[r]) * (ld - 1), int(host["n_notes"][r])
        assert 0 <= n <= (int(seg_first[r + 1]) - int(seg_first[r])) * (ld - 1)
        result.append(notes.NoteArrays(host["times"].reshape(-1, 2)[a:a + n], host["meta"].reshape(-1, 4)[a:a + n],
                                       host["logc"][a:a + n] if scored else None, int(host["invalid"][r]),
                                       int(host["dropped"][r]), float(host["total"][r]), int(host["status"][r])))
    return result


def _check(batch, scored, dev):
    got = _launch(batch, scored, dev)
    for case, arrays in zip(batch, got):
        assert arrays.status == 0, (case.name, "left to the fallback")
        N.same_arrays(arrays, N.host_arrays(case, scored), "%s ld %d%s" % (case.name, case.ids.shape[1], " scored" * scored))
    return got


@pytest.mark.parametrize("scored", [False, True])
def test_kernel_equals_the_host_restatement(cases, dev, scored):
    """The whole corpus and every hand-written case as the recordings of ONE launch (unequal row counts, the common row
    length), every recording exact and none left to the fallback; the hand-written cases give their known answers."""
    from mrmt3 import lib
    ld = max(c.ids.shape[1] for c in cases)
    batch = [_fit(c, ld) for c in cases]
    before = lib.notes_launches()
    got = _check(batch, scored, dev)
    assert lib.notes_launches() == before + 1
    for case, arrays in zip(cases, got):
        if case.expect is not None:
            N.check_expectation(case, arrays)
    print("[device notes] %d recordings, %d rows of %d, %d notes" % (len(batch), sum(len(c.ids) for c in batch), ld,
                                                                    sum(len(a) for a in got)))


@pytest.mark.parametrize("ld", [2, 9, 64])
def test_row_lengths_and_recording_counts(cases, dev, ld):
    """Rows of `ld` columns: one recording alone, three of unequal row counts in one launch, and the whole corpus cut to it."""
    by_rows = {}
    for c in cases:
        by_rows.setdefault(len(c.ids), []).append(c)
    assert {1, 3, 7} <= set(by_rows)
    _check([_fit(by_rows[7][1], ld)], True, dev)
    _check([_fit(by_rows[7][2], ld)], False, dev)
    _check([_fit(by_rows[n][3], ld) for n in (3, 7, 1)], True, dev)
    got = _check([_fit(c, ld) for c in cases], True, dev)
    assert ld == 2 or sum(len(a) for a in got) > 0


def test_a_dense_recording_of_full_rows(dev):
    """7 rows of 1024 columns, every row full to its last column: four chunks a row, the step count carried between them."""
    case = N.dense_case()
    for scored in (False, True):
        got = _check([case], scored, dev)[0]
        assert len(got) > 1000


def _capacity_case(programs, then=()):
    """One row striking 128 pitches of each of `programs` programs, then the tokens `then`."""
    rng = np.random.RandomState(11)
    row = [N.TIE, N.ON]
    for g in range(programs):
        row += [N.G(g)] + [N.P(p) for p in range(128)]
    return N._case("%d programs" % programs, [row + list(then) + [N.EOS]], rng)


def test_capacity(dev):
    """More notes sounding at once than the capacity: the kernel says so, `decode_notes` returns the host's result for that
    recording and the kernel's for its small neighbour.  Exactly the capacity, then offs and fresh onsets: exact."""
    from mrmt3 import lib, notes
    assert lib.NOTES_CAPACITY == 4096
    over, small = _capacity_case(33), N.hand_cases()[0]
    small = _fit(small, over.ids.shape[1])
    raw = _launch([over, small], True, dev)
    assert [a.status for a in raw] == [notes.STATUS_CAPACITY, 0]
    N.same_arrays(raw[1], N.host_arrays(small, True), "beside a recording over capacity")
    before = lib.notes_launches()
    up = lambda a: torch.from_numpy(a).to(dev)
    got = notes.decode_notes(up(np.concatenate([over.ids, small.ids])), np.concatenate([over.frames, small.frames])[:, None],
                             N.CODEC, logp=up(np.concatenate([over.logp, small.logp])), recordings=[1, 1])
    assert lib.notes_launches() == before + 1 and [a.status for a in got] == [notes.STATUS_CAPACITY, 0]
    want = N.host_arrays(over, True)
    assert len(want) == 33 * 128
    got[0].status = 0
    N.same_arrays(got[0], want, "the fallback")
    N.same_arrays(got[1], raw[1], "the neighbour")
    # a full list with dead slots is compacted, not refused
    then = [N.OFF] + [N.P(p) for p in range(0, 20, 2)] + [N.ON] + [N.P(p) for p in range(0, 10, 2)] + \
           [N.G(40)] + [N.P(p) for p in range(5)]
    for scored in (True, False):
        assert len(_check([_capacity_case(32, then)], scored, dev)[0]) == 4096 + 10
    assert _launch([_capacity_case(32, then + [N.P(5)])], False, dev)[0].status == notes.STATUS_CAPACITY


def test_argument_errors_launch_nothing(cases, dev):
    from mrmt3 import lib
    batch = [_fit(cases[0], 16)]
    g = N.grammar()
    before = lib.notes_launches()
    bad = [dict(rows=0), dict(rows=-1), dict(ld=1), dict(ld=0), dict(n_rec=0), dict(n_rec=-2)]
    bad += [{k: None} for k in ("g", "ids", "seg_first", "start", "limit", "vel", "n_notes", "invalid", "dropped", "status",
                                "total", "times", "meta")]
    for over in bad:
        assert _launch(batch, False, dev, expect_rc=1, **over) is None, over
    assert _launch(batch, True, dev, expect_rc=1, logc=None) is None              # logp without logc
    for field in (dict(n_pitch=129), dict(n_program=129), dict(steps_per_second=0), dict(steps_per_second=-100)):
        assert _launch(batch, False, dev, grammar=dataclasses.replace(g, **field), expect_rc=1) is None, field
    assert lib.notes_launches() == before
    with pytest.raises(RuntimeError, match="notes_decode_fwd"):
        z = torch.zeros(2, 1, dtype=torch.int64, device=dev)
        lib.notes_decode(g, z, torch.tensor([0, 2], dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.float64, device=dev),
                         torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), 100)
    assert lib.notes_launches() == before


def test_decode_notes_from_frame_times(cases, dev):
    """The Python layer: start times and limits from frame times, several recordings, the compact copy back."""
    from mrmt3 import notes
    some = [c for c in cases if c.frames is not None][:40]
    ld = max(c.ids.shape[1] for c in some)
    batch = [_fit(c, ld) for c in some]
    up = lambda a: torch.from_numpy(a).to(dev)
    for scored in (False, True):
        got = notes.decode_notes(up(np.concatenate([c.ids for c in batch])), np.concatenate([c.frames for c in batch])[:, None],
                                 N.CODEC, logp=up(np.concatenate([c.logp for c in batch])) if scored else None,
                                 recordings=[len(c.ids) for c in batch])
        for case, arrays in zip(batch, got):
            N.same_arrays(arrays, N.host_arrays(case, scored), case.name)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _model(variant, dev):
    from mrmt3.synthetic import T5_SMALL
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        m = T5ForConditionalGeneration(T5_SMALL, compute_dtype=torch.float32)
    else:
        from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
        m = T5SegMemV2WithPrev(T5_SMALL, segmem_num_layers=1, segmem_length=64, compute_dtype=torch.float32)
    return m.load_golden().to(dev).eval()


class _EndsRows:
    """The model, except that every id row it returns begins `tie, velocity-on, drum, program, pitch` (drum, program and
    pitch vary with the row) and holds EOS in column `at`: an untrained model never ends a row, a row without EOS
    contributes no tokens, and what it does emit hardly ever makes a note.  Everything else — the other ids, the
    log-probabilities, where they live — is the decoder's own."""

    def __init__(self, model, at):
        self._model, self._at = model, at

    def _end(self, x):
        if isinstance(x, (tuple, list)):
            return type(x)(self._end(v) for v in x)
        if torch.is_tensor(x) and x.dtype == torch.int64 and x.dim() == 2 and x.shape[1] > self._at > 5:
            x = x.clone()
            r = torch.arange(x.shape[0], device=x.device)
            x[:, 1], x[:, 2], x[:, 3], x[:, 4], x[:, 5] = N.TIE, N.ON, N.D(36) + r % 8, N.G(0) + r % 3, N.P(60) + r % 5
            x[:, self._at] = N.EOS
        return x

    def __getattr__(self, name):
        attr = getattr(self._model, name)
        if not name.startswith("generate"):
            return attr
        return lambda *args, **kw: self._end(attr(*args, **kw))


def _same_sequence(a, b):
    assert a.notes == b.notes and a.total_time == b.total_time
    assert [(n.instrument, n.confidence) for n in a.notes] == [(n.instrument, n.confidence) for n in b.notes]


def test_inference_end_to_end(dev, tmp_path):
    """`inference(device_notes=True)` returns the note sequence of the host path, plain, scored with a floor, constrained;
    one launch per call; switched off, nothing is launched and the other kernels are launched as before."""
    import inference
    from contrib import midi_io
    from mrmt3 import lib
    from mrmt3.synthetic import synth_audio
    m = _EndsRows(_model("t5", dev), 46)
    m.engine.prepare(False)
    h = inference.InferenceHandler(model=m, device=dev, decode_options=True)
    assert h.device_notes is False
    audio = synth_audio(1, n_samples=7 * 32768 + 1000, seed=9)[0]
    lib.notes_launches(reset=True)
    n_notes = 0
    for kw in (dict(), dict(with_confidence=True, min_confidence=0.5), dict(with_confidence=True), dict(constrained=True),
               dict(constrained=True, with_confidence=True, batch_size=3)):
        lib.dispatch_counts(reset=True)
        host = h.inference(audio, max_length=48, **kw)
        counts = lib.dispatch_counts(reset=True)
        assert lib.notes_launches() == 0
        device = h.inference(audio, max_length=48, device_notes=True, **kw)
        assert lib.notes_launches(reset=True) == 1 and lib.dispatch_counts() == counts
        _same_sequence(device, host)
        n_notes += len(host.notes)
    print("[device notes] end to end: %d notes" % n_notes)
    assert n_notes > 0
    toks = h.inference(audio, max_length=48, return_tokens=True, device_notes=True)       # ignores the keyword
    assert lib.notes_launches() == 0 and all(np.array_equal(a, b) for a, b in zip(toks[0], h.inference(
        audio, max_length=48, return_tokens=True)[0]))
    on = inference.InferenceHandler(model=m, device=dev, decode_options=True, device_notes=True)
    out_a, out_b = str(tmp_path / "a.mid"), str(tmp_path / "b.mid")
    _same_sequence(on.inference(audio, max_length=48, constrained=True, outpath=out_a),
                   h.inference(audio, max_length=48, constrained=True, outpath=out_b))
    assert lib.notes_launches(reset=True) == 1 and open(out_a, "rb").read() == open(out_b, "rb").read()
    assert on.inference(audio, max_length=48, device_notes=False) is not None and lib.notes_launches() == 0


def test_inference_many_end_to_end(dev):
    """Two recordings of unequal length through a segment-memory model: one launch for both."""
    import inference
    from mrmt3 import lib
    from mrmt3.synthetic import synth_audio
    m = _EndsRows(_model("segmem", dev), 46)
    m.engine.prepare(False)
    h = inference.InferenceHandler(model=m, device=dev, decode_options=True)
    audio = synth_audio(1, n_samples=4 * 32768, seed=9)[0]
    audios = [audio, audio[:50000]]
    lib.notes_launches(reset=True)
    n_notes = 0
    for kw in (dict(), dict(with_confidence=True, min_confidence=0.5), dict(constrained=True, with_confidence=True)):
        host = h.inference_many(audios, max_length=48, **kw)
        assert lib.notes_launches() == 0
        device = h.inference_many(audios, max_length=48, device_notes=True, **kw)
        assert lib.notes_launches(reset=True) == 1 and len(device) == len(host) == 2
        for a, b in zip(device, host):
            _same_sequence(a, b)
        print("[device notes] inference_many %s: %s notes" % (kw, [len(x.notes) for x in host]))
        n_notes += sum(len(x.notes) for x in host)
    assert n_notes > 0
