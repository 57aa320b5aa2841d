"""The device resampler without a GPU: the polyphase table and the contract's numpy restatement
(tests/_resample.py) against scipy's resample_poly and the analytic sine, the restatement's own properties (a crop is a
slice, pass-through is `mix_rows`), the labels of a pitch-shifted track against their definition, the plan's draw order,
and every host validation."""
import ctypes
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import _resample as rsm
import _stem_mix as sm
from test_stem_mix_cpu import _Recorder

HOP = 128
ONE = 1 << 32
TONES = (440, 3000, 5000, 6000, 9000, 12000)          # pass band ... | stop band: 9000, 12000 (6.5 - 8 kHz: transition)


# ---- quality against an independent reference -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def scipy_errors():
    """Max error of scipy.signal.resample_poly(x, 160, 441) on each tone (1 s at 44100 Hz, 400 samples cut per edge)."""
    from scipy.signal import resample_poly
    return {f: rsm.tone_errors(lambda x: resample_poly(x.astype(np.float64), 160, 441), f, 44100, 16000, 44100)
            for f in TONES}


def test_restatement_is_no_worse_than_scipy_on_every_tone(scipy_errors):
    from mrmt3.resample import ratio_step, resample_filter
    step = ratio_step(Fraction(44100, 16000))
    h = resample_filter(Fraction(step, ONE))
    assert h.dtype == np.float32 and h.shape == (513, 94)
    assert np.array_equal(h[512, 1:], h[0, :-1]) and h[512, 0] == 0              # row P = row 0 shifted by one sample
    for f in TONES:
        err = rsm.tone_errors(lambda x: rsm.resample_1d(x, step, h), f, 44100, 16000, 44100)
        print("tone %5d Hz: restatement %.3g, scipy %.3g" % (f, err, scipy_errors[f]))
        assert err <= scipy_errors[f], (f, err, scipy_errors[f])


@pytest.mark.parametrize("k, taps", [(3, 42), (-3, 36)])
def test_a_pitch_shifted_tone_is_the_analytic_sine(scipy_errors, k, taps):
    from mrmt3.resample import out_length, ratio_step, resample_filter
    step = ratio_step(2.0 ** (k / 12.0))
    h = resample_filter(Fraction(step, ONE))
    assert h.shape == (513, taps)
    x = np.sin(2 * np.pi * 3000 * np.arange(16000) / 16000).astype(np.float32)
    y = rsm.resample_1d(x, step, h).astype(np.float64)
    assert len(y) == out_length(16000, step)
    want = np.sin(2 * np.pi * 3000 * np.arange(len(y)) * (step / ONE) / 16000)
    err = float(np.abs(y - want)[400:-400].max())
    print("k = %+d: %.3g (bound %.3g)" % (k, err, max(scipy_errors.values())))
    assert err <= max(scipy_errors.values())


def test_filter_tables_of_unequal_width_stack_symmetrically():
    from mrmt3.resample import resample_filter, stack_filters
    a, b = resample_filter(2.0 ** (-3 / 12)), resample_filter(2.0 ** (3 / 12))
    st = stack_filters([a, b])
    assert st.shape == (2, 513, 42) and np.array_equal(st[1], b)
    assert np.array_equal(st[0, :, 3:39], a) and not st[0, :, :3].any() and not st[0, :, 39:].any()
    # the padded table computes the same row, bit for bit (the extra taps hold +0 coefficients)
    x = np.random.RandomState(0).uniform(-1, 1, 600).astype(np.float32)
    step = 3611622603
    assert np.array_equal(rsm.resample_1d(x, step, a), rsm.resample_1d(x, step, st[0]))


# ---- properties of the restatement ----------------------------------------------------------------------------------

def test_a_crop_is_a_slice_of_one_long_row():
    from mrmt3.resample import ratio_step, resample_filter
    rs = np.random.RandomState(1)
    pool = np.concatenate([np.full(7, np.nan, np.float32), rs.uniform(-1, 1, 3000).astype(np.float32),
                           np.full(5, np.nan, np.float32)])
    a = lambda v: np.array([[v]], np.int64)
    for ratio in (2.0 ** (3 / 12), 2.0 ** (-3 / 12), Fraction(44100, 16000)):
        step = ratio_step(ratio)
        filt = resample_filter(Fraction(step, ONE))[None]
        n_long = ((3000 - 1) << 32) // step + 40                                # runs past the stem's end
        g = np.full((1, 1), 0.75, np.float32)
        long = rsm.resample_rows(pool, a(7 << 32), a(7), a(3007), a(step), g, a(0), n_long, filt)[0]
        assert np.isfinite(long).all() and long[-1] == 0 and long[:100].any()
        for s in (0, 1, 129, n_long - 300):
            crop = rsm.resample_rows(pool, a((7 << 32) + s * step), a(7), a(3007), a(step), g, a(0), 300, filt)[0]
            assert np.array_equal(crop.view(np.int32), long[s:s + 300].view(np.int32)), (ratio, s)


def test_pass_through_tables_are_mix_rows():
    c = sm.stem_case(5, 300)
    want = sm.mix_rows(c["pool"], c["start"], c["end"], c["gain"], 300, c["hop"], c["valid_frames"])
    thru = np.full(c["gain"].shape, -1)
    got = rsm.resample_rows(c["pool"], c["start"] << 32, c["start"], c["end"], np.full(c["gain"].shape, ONE), c["gain"],
                            thru, 300, np.zeros((0, 513, 2), np.float32), c["valid_frames"].astype(np.int64) * c["hop"])
    assert want.any() and np.array_equal(got.view(np.int32), want.view(np.int32))
    # the fraction of a pass-through position is ignored
    got = rsm.resample_rows(c["pool"], (c["start"] << 32) + 12345, c["start"], c["end"], np.full(c["gain"].shape, ONE),
                            c["gain"], thru, 300, np.zeros((0, 513, 2), np.float32),
                            c["valid_frames"].astype(np.int64) * c["hop"])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_restatement_skips_what_the_contract_skips():
    from mrmt3.resample import resample_filter, stack_filters
    c = rsm.resample_case(5, 300, [3611622603, 5107599035], passthrough=(2,))
    filt = stack_filters([resample_filter(Fraction(3611622603, ONE)), resample_filter(Fraction(5107599035, ONE))])
    rows = rsm.resample_rows(c["pool"], c["pos"], c["begin"], c["end"], c["step"], c["gain"], c["filt_idx"], 300, filt,
                             c["valid_samples"])
    assert np.isfinite(rows).all(), "a NaN gap was read"
    assert rows[0].any() and not rows[1, int(c["valid_samples"][1]):].any() and rows[1, :int(c["valid_samples"][1])].any()
    # a filter index outside [-1, n_filt), a step <= 0 and begin >= end silence a source; so does gain 0
    base = dict(c)
    for key, val in (("filt_idx", 2), ("filt_idx", -2), ("step", 0), ("step", -5), ("begin", None)):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        if key == "begin":
            d["begin"][:, 0] = d["end"][:, 0]
        else:
            d[key][:, 0] = val
        muted = dict(base, gain=base["gain"].copy())
        muted["gain"][:, 0] = 0
        got = rsm.resample_rows(d["pool"], d["pos"], d["begin"], d["end"], d["step"], d["gain"], d["filt_idx"], 300, filt)
        want = rsm.resample_rows(c["pool"], c["pos"], c["begin"], c["end"], c["step"], muted["gain"], c["filt_idx"], 300, filt)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (key, val)


# ---- labels -----------------------------------------------------------------------------------------------------------

def _onsets(tok, feats):
    """[(step, event type, value)] of every pitch / drum token of a tokenisation, the step counted in `shift 1` tokens."""
    out, steps, vel = [], 0, 1
    for e in feats["targets"]:
        ev = tok.codec.decode_event_index(int(e))
        if ev.type == "shift":
            steps += ev.value
        elif ev.type == "velocity":
            vel = ev.value
        elif ev.type in ("pitch", "drum") and vel > 0:
            out.append((steps, ev.type, ev.value))
    return out


def test_speed_note_sequence_moves_onsets_and_transposes_pitched_notes_only():
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.resample import ratio_step
    from mrmt3.stems import speed_note_sequence
    from mrmt3.tokenizer import Tokenizer
    ns = NoteSequence(notes=[Note(1.234, 1.9, 60, 90, 0, False, 0), Note(2.5, 2.6, 38, 90, 0, True, 1)], total_time=2.6)
    step = ratio_step(2.0 ** (2 / 12.0))
    fast = speed_note_sequence(ns, 2, step)
    scale = float(ONE) / float(step)
    assert [(n.start_time, n.end_time, n.pitch) for n in fast.notes] == [(1.234 * scale, 1.9 * scale, 62), (2.5 * scale, 2.6 * scale, 38)]
    assert fast.total_time == 2.6 * scale and ns.notes[0].pitch == 60 and ns.notes[0].start_time == 1.234     # copies
    tok = Tokenizer()
    got = _onsets(tok, tok.tokenize(fast, 4 * 16000))
    sps = tok.codec.steps_per_second
    assert (round(1.234 * scale * sps), "pitch", 62) in got and (round(2.5 * scale * sps), "drum", 38) in got
    assert not any(t == "pitch" and v == 60 for _, t, v in got)


def _batcher(**kw):
    from mrmt3.batching import StemMixBatcher
    return StemMixBatcher("cpu", mel_length=64, event_length=256, num_rows_per_batch=4, split_frame_length=100, **kw)


def test_shift_is_clamped_to_the_tracks_pitches():
    from mrmt3.stems import shift_range

    class Up:
        def __getattr__(self, name):
            return getattr(random.Random(3), name)

        def randint(self, a, b):
            return b if (a, b) == (-5, 5) else random.Random(3).randint(a, b)

    tr = sm.synthetic_tracks(1)[0]
    lo, hi = shift_range(tr)
    assert (lo, hi) == (-min(n.pitch for s in (0, 2) for n in tr.notes[s].notes), 127 - max(n.pitch for s in (0, 2) for n in tr.notes[s].notes))
    assert _batcher(pitch_shift=5, rng=Up()).plan(tr).shift == 5
    tr.notes[0].notes[0].pitch = 126
    tr.notes[1].notes[0].pitch = 127                                  # a drum note does not count
    assert shift_range(tr)[1] == 1
    plan = _batcher(pitch_shift=5, rng=Up()).plan(tr)
    from mrmt3.resample import ratio_step
    assert plan.shift == 1 and plan.step == ratio_step(2.0 ** (1 / 12.0))


def test_plan_draws_the_shift_first_and_nothing_else_changes():
    from mrmt3.batching import plan_stem_mix
    from mrmt3.resample import out_length, ratio_step
    tr = sm.synthetic_tracks(1)[0]
    geom = dict(mel_length=64, num_rows_per_batch=4, split_frame_length=100)
    # pitch_shift = 0: exactly the parent's stream (plan_stem_mix over the track's frames), and the default plan fields
    rec0, rec1 = _Recorder(11), _Recorder(11)
    p0 = _batcher(rng=rec0).plan(tr)
    p1 = plan_stem_mix(-(-tr.n_samples // HOP), 3, rng=rec1, **geom)
    assert rec0.log == rec1.log and len(rec0.log) > 5 and (p0.shift, p0.step) == (0, ONE)
    assert np.array_equal(p0.crops.start_frame, p1.crops.start_frame) and np.array_equal(p0.gain, p1.gain)
    # pitch_shift = 4: one randint(-4, 4) first, then the parent's draws over the stretched track's frames
    rec = _Recorder(11)
    p = _batcher(pitch_shift=4, rng=rec).plan(tr)
    assert rec.log[0][:3] == ("randint", -4, 4) and p.shift == rec.log[0][3] != 0
    assert p.step == ratio_step(2.0 ** (p.shift / 12.0))
    frames = -(-max(out_length(len(a), p.step) for a in tr.audio) // HOP)
    assert frames != -(-tr.n_samples // HOP)

    class After(_Recorder):
        def __init__(self, seed):
            super().__init__(seed)
            self.r.randint(-4, 4)                                     # (the same generator, one draw further)

    ref = After(11)
    q = plan_stem_mix(frames, 3, rng=ref, **geom)
    assert rec.log[1:] == ref.log and np.array_equal(p.crops.start_frame, q.crops.start_frame) and np.array_equal(p.gain, q.gain)
    # the deterministic (validation) form draws nothing and is never shifted
    det = _batcher(pitch_shift=4, is_deterministic=True, rng=_Recorder(1)).plan(tr)
    assert (det.shift, det.step) == (0, ONE)
    for bad in (-1, 2.5, True, 25):
        with pytest.raises(ValueError, match="pitch_shift"):
            _batcher(pitch_shift=bad)


def test_cached_targets_of_a_shifted_plan_equal_the_definition():
    from mrmt3.stems import merged_note_sequence, speed_note_sequence

    class Forced(random.Random):
        def __init__(self, k):
            super().__init__(9)
            self.k, self.first = k, True

        def randint(self, a, b):
            if self.first:
                self.first = False
                return self.k
            return super().randint(a, b)

    tr = sm.synthetic_tracks(1)[0]
    for k in (3, -2):
        b = _batcher(pitch_shift=3, rng=Forced(k))
        plan = b.plan(tr)
        assert plan.shift == k
        got = b.row_targets(tr, plan)
        again = b.row_targets(tr, plan)                                # served from the cache
        n_long = b.n_samples(tr, plan.step)
        assert n_long == max(((len(a) - 1) << 32) // plan.step + 1 for a in tr.audio)
        for r in range(len(got)):
            kept = tuple(int(s) for s in np.nonzero(plan.keep[r])[0])
            feats = b.tokenizer.tokenize(speed_note_sequence(merged_note_sequence(tr, kept), k, plan.step), n_long)
            want = b.tokenizer.row_targets(feats, int(plan.crops.start_frame[r]), int(plan.crops.valid_frames[r]))
            assert np.array_equal(got[r], want) and np.array_equal(again[r], want) and len(want) > 0
        assert all(key[2] == k for key in b._feats)


def test_shifted_tables_follow_the_plan():
    from mrmt3.batching import StemMixPlan, CropPlan, resample_tables, stem_pool_layout
    from mrmt3.resample import check_resample_tables, out_length, ratio_step
    step = ratio_step(2.0 ** (3 / 12.0))
    lengths = [3000, 1000, 2000]
    offsets, total = stem_pool_layout(lengths, HOP)
    last = out_length(1000, step)                                      # stretched samples of the short stem
    starts = np.array([0, last // HOP, -(-last // HOP), 12], np.int64)
    plan = StemMixPlan(CropPlan(starts, np.array([4, 4, 4, 2], np.int32), np.zeros(4, np.int64)), np.ones((4, 3), bool),
                       np.full((4, 3), 0.5, np.float32), 3, step)
    pos, begin, end, st, gain, filt, valid = resample_tables(plan, offsets, lengths, HOP)
    assert np.array_equal(begin[0], offsets) and np.array_equal(end[0], offsets + lengths) and (st == step).all()
    assert np.array_equal(pos[:, 0], (offsets[0] << 32) + starts * HOP * step)
    assert gain[1, 1] == 0.5 and gain[2, 1] == 0 and pos[2, 1] == offsets[1] << 32       # at or behind the stem's end: silent
    assert gain[3, 1] == 0 and gain[3, 2] == 0.5 and not filt.any() and valid.tolist() == [512, 512, 512, 256]
    assert plan.gain[2, 1] == 0.5                                                        # the labels are untouched
    check_resample_tables(pos, begin, end, st, gain, filt, total, 1)
    # every source that is left sounding has its first tap inside its stem
    first = (pos >> 32) - 42 // 2 + 1
    assert (first[gain != 0] < end[gain != 0]).all()


# ---- host validation ------------------------------------------------------------------------------------------------

def test_ratio_step_and_out_length():
    from mrmt3.resample import out_length, ratio_step
    assert ratio_step(1) == ONE and ratio_step(0.25) == ONE // 4 and ratio_step(4.0) == 4 * ONE
    assert ratio_step(Fraction(44100, 16000)) == round(Fraction(44100, 16000) * ONE) == 11838003610
    for bad in (0.2499, 4.0001, 0, -1, float("nan"), float("inf"), "fast"):
        with pytest.raises(ValueError, match="ratio"):
            ratio_step(bad)
    assert out_length(1, ONE) == 1 and out_length(100, ONE) == 100 and out_length(100, 2 * ONE) == 50
    assert out_length(101, 2 * ONE) == 51 and out_length(100, ONE // 2) == 199


def test_check_resample_tables_names_the_row():
    from mrmt3.resample import check_resample_tables
    step = 5107599035
    ok = dict(pos=np.array([[10 << 32, (50 << 32) + 7], [(12 << 32) + 1, 60 << 32]], np.int64),
              begin=np.array([[0, 40], [0, 40]], np.int64), end=np.array([[30, 90], [30, 90]], np.int64),
              step=np.array([[step, step], [step, ONE]], np.int64), gain=np.array([[1, 0.5], [2, 1]], np.float32),
              filt=np.array([[0, 1], [0, -1]], np.int32))
    order = ("pos", "begin", "end", "step", "gain", "filt")
    check_resample_tables(*(ok[k] for k in order), 100, 2)

    def bad(match, **change):
        t = {k: v.copy() for k, v in ok.items()}
        for k, (at, v) in change.items():
            t[k][at] = v
        with pytest.raises(ValueError, match=match):
            check_resample_tables(*(t[k] for k in order), 100, 2)

    bad("row 1 has a gain that is not finite", gain=((1, 0), np.inf))
    bad("row 0 has a gain that is not finite", gain=((0, 1), np.nan))
    bad("row 1 points outside the pool", end=((1, 1), 101))
    bad("row 0 points outside the pool", begin=((0, 0), -1))
    bad("row 1 points outside the pool", begin=((1, 0), 31))                   # begin > end
    bad("row 0 starts outside its stem", pos=((0, 1), 39 << 32))
    bad("row 1 starts outside its stem", pos=((1, 0), 31 << 32))
    bad("row 0 has a step outside", step=((0, 0), ONE // 4 - 1))
    bad("row 1 has a step outside", step=((1, 0), 4 * ONE + 1))
    bad("row 1 has a step outside", step=((1, 0), 0))
    bad("row 0 names a filter outside", filt=((0, 1), 2))
    bad("row 1 names a filter outside", filt=((1, 1), -2))
    bad("row 1 passes a source through", step=((1, 1), step))
    bad("row 1 passes a source through", pos=((1, 1), (60 << 32) + 1))
    # a silent source is not looked at; shapes and the source count are
    t = {k: v.copy() for k, v in ok.items()}
    t["gain"][1, 1], t["end"][1, 1], t["filt"][1, 1], t["step"][1, 1] = 0, 10 ** 12, 99, -3
    check_resample_tables(*(t[k] for k in order), 100, 2)
    with pytest.raises(ValueError, match="share one"):
        check_resample_tables(ok["pos"], ok["begin"], ok["end"][:1], ok["step"], ok["gain"], ok["filt"], 100, 2)
    wide = [np.zeros((1, 65), np.int64)] * 4 + [np.zeros((1, 65), np.float32), np.zeros((1, 65), np.int32)]
    with pytest.raises(ValueError, match="65 sources"):
        check_resample_tables(*wide, 100, 2)


def test_the_entry_point_is_declared_bound_and_refuses_bad_arguments_without_a_device():
    from mrmt3 import lib
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert lib._SIGS["mrmt3_resample_mix_fwd"] == (ci, [vp, ll, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, vp, vp, vp])
    assert lib._SIGS["mrmt3_resample_launches"] == (ctypes.c_ulonglong, [ci])
    so = lib.load()
    assert so.mrmt3_version() >= 124 and lib.MIN_VERSION >= 124 and callable(lib.resample_mix)
    buf = (ctypes.c_double * 8)()
    a = (ctypes.addressof(buf) + 15) & ~15
    lib.resample_launches(reset=True)
    good = [a, 100, a, a, a, a, a, a, 2, 3, 300, a, 1, 42, None, a, None]
    names = ("pool", "pool_samples", "src_pos", "src_begin", "src_end", "src_step", "src_gain", "src_filt", "n_src",
             "batch", "n_samples", "filt", "n_filt", "n_taps", "valid_samples", "out", "stream")
    cases = [(n, None, b"null") for n in ("pool", "src_pos", "src_begin", "src_end", "src_step", "src_gain", "src_filt",
                                          "filt", "out")]
    cases += [("n_src", 0, b"n_src"), ("n_src", 65, b"n_src"), ("n_taps", 41, b"n_taps"), ("n_taps", 0, b"n_taps"),
              ("n_taps", 162, b"n_taps"), ("n_filt", -1, b"n_filt"), ("pool_samples", 0, b"sizes"), ("batch", 0, b"sizes"),
              ("n_samples", 0, b"sizes"), ("n_samples", -4, b"sizes"), ("filt", a + 4, b"aligned")]
    for name, val, word in cases:
        args = list(good)
        args[names.index(name)] = val
        assert so.mrmt3_resample_mix_fwd(*args) == 1 and word in so.mrmt3_last_error(), (name, val, so.mrmt3_last_error())
    assert lib.resample_launches() == 0                                  # nothing was launched


def test_train_py_validates_the_two_new_stem_options(tmp_path):
    from mrmt3 import hydra_lite
    from test_config_cpu import MODEL, TOP
    import train
    (tmp_path / "model").mkdir()
    (tmp_path / "dataset").mkdir()
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    comp = lambda *over: hydra_lite.compose(str(tmp_path), "config", list(over))
    got = train.stem_options(comp("+stem_root=/d", "+stem_pitch_shift=3", "+stem_native_rate=true"))
    assert got["pitch_shift"] == 3 and got["native_rate"] is True and got["keep"] == 0.75
    assert train.stem_options(comp("+stem_root=/d", "+stem_pitch_shift=0", "+stem_native_rate=false")) == dict(
        root="/d", val_root=None, keep=0.75, gain_db=6.0, min_stems=1, pitch_shift=0, native_rate=False)
    for over, match in (("+stem_pitch_shift=-1", "stem_pitch_shift"), ("+stem_pitch_shift=1.5", "stem_pitch_shift"),
                        ("+stem_pitch_shift=high", "stem_pitch_shift"), ("+stem_pitch_shift=25", "stem_pitch_shift"),
                        ("+stem_pitch_shift=true", "stem_pitch_shift"), ("+stem_native_rate=2", "stem_native_rate"),
                        ("+stem_native_rate=maybe", "stem_native_rate")):
        with pytest.raises(ValueError, match=match):
            train.stem_options(comp("+stem_root=/d", over))
    assert train.stem_options(comp("+stem_pitch_shift=3")) is None        # without +stem_root nothing changes


def test_load_track_accepts_another_rate_only_when_asked(tmp_path):
    from contrib import audio_io
    from mrmt3 import stems
    from mrmt3.resample import out_length, ratio_step
    src = sm.synthetic_tracks(1)
    root = sm.write_tracks(tmp_path / "root", src)
    d = os.path.join(root, "track00")
    for name, a in zip(src[0].stem_names, src[0].audio):
        audio_io.write_wav(os.path.join(d, "stems", name + ".wav"), a, sr=22050)
    with pytest.raises(ValueError, match=r"s0\.wav.*22050"):
        stems.load_track(d)
    with pytest.raises(ValueError, match=r"s0\.wav.*22050"):
        stems.load_stem_folder(root)
    tr = stems.load_stem_folder(root, any_rate=True)[0]
    assert tr.rates == [22050] * 3 and [len(a) for a in tr.audio] == [len(a) for a in src[0].audio]
    step = ratio_step(Fraction(22050, 16000))
    assert tr.lengths(16000) == [out_length(len(a), step) for a in src[0].audio] and tr.n_samples == max(tr.lengths())
    assert tr.lengths(22050) == [len(a) for a in src[0].audio]
    assert [n.start_time for n in tr.notes[0].notes][:3] == [n.start_time for n in stems.load_track(d, 22050).notes[0].notes][:3]
    assert stems.load_track(d, 22050).rates is None                      # at the config's rate: as before
    audio_io.write_wav(os.path.join(d, "stems", "s1.wav"), src[0].audio[1], sr=3000)
    with pytest.raises(ValueError, match=r"s1\.wav.*3000.*1/4"):
        stems.load_track(d, any_rate=True)
