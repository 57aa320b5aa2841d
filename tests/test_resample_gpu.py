"""The device resampler on a real MI355X: mrmt3_resample_mix_fwd against the contract's numpy restatement
(tests/_resample.py) bit for bit, its pass-through form against the stem-mix launch, `mrmt3.resample.resample` against
scipy, the argument checks, then pitch-shift rows and native-rate stems in the batcher, train.py and the inference handler."""
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import _resample as rsm
import _stem_mix as sm

pytestmark = pytest.mark.gpu

HOP = 128
ONE = 1 << 32
TILE = 1024                                            # outputs per workgroup (csrc/resample.hip: RS_TILE)
SIZES = [300, TILE + 37]                               # inside one tile; across a tile boundary with a ragged tail
TONES = (440, 3000, 5000, 6000, 9000, 12000)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bank():
    """(steps, tables [4, 513, 94]): 2^(3/12), 2^(-3/12), 44100 / 16000 and 1/2, each with its own filter."""
    from mrmt3.resample import ratio_step, resample_filter, stack_filters
    steps = [ratio_step(2.0 ** (3 / 12.0)), ratio_step(2.0 ** (-3 / 12.0)), ratio_step(Fraction(44100, 16000)), ONE // 2]
    return steps, stack_filters([resample_filter(Fraction(s, ONE)) for s in steps])


def _bits(x):
    x = x.cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32).numpy()


def _launch(c, filt, dev, valid="case", n_samples=None):
    """One counted launch of the kernel on a `resample_case`-style dict."""
    from mrmt3 import lib
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    valid = c["valid_samples"] if isinstance(valid, str) else valid
    before = lib.resample_launches()
    out = lib.resample_mix(t(c["pool"], np.float32), t(c["pos"], np.int64), t(c["begin"], np.int64), t(c["end"], np.int64),
                           t(c["step"], np.int64), t(c["gain"], np.float32), t(c["filt_idx"], np.int32),
                           n_samples or c["n_samples"], t(filt, np.float32), None if valid is None else t(valid, np.int64))
    torch.cuda.synchronize()
    assert lib.resample_launches() == before + 1
    return out.cpu().numpy()


def _restated(c, filt, valid="case", n_samples=None):
    valid = c["valid_samples"] if isinstance(valid, str) else valid
    return rsm.resample_rows(c["pool"], c["pos"], c["begin"], c["end"], c["step"], c["gain"], c["filt_idx"],
                             n_samples or c["n_samples"], filt, valid)


def _check_case(c, filt, dev):
    want = _restated(c, filt)
    got = _launch(c, filt, dev)
    assert np.isfinite(got).all(), "something between the stems was read"
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    v = int(c["valid_samples"][1])
    assert want[0].any() and want[1, :v].any() and not got[1, v:].any()          # short row: the tail is exactly 0
    full = _launch(c, filt, dev, valid=None)                                     # ... and without valid_samples it is not
    assert np.array_equal(_bits(full), _bits(_restated(c, filt, valid=None))) and full[1, v:].any()


# ---- 6. the kernel equals the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_samples", SIZES)
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_one_source_equals_the_restatement(dev, bank, which, n_samples):
    steps, filt = bank
    c = rsm.resample_case(1, n_samples, steps[which:] + steps[:which], seed=which)
    c["filt_idx"] = (c["filt_idx"] + which) % 4                                  # (the case numbers filters by position)
    _check_case(c, filt, dev)


@pytest.mark.parametrize("n_samples", SIZES)
@pytest.mark.parametrize("passthrough", [(), (1, 4)])
def test_five_sources_equal_the_restatement(dev, bank, passthrough, n_samples):
    """Every step in one row, a gain-0 source that points into a NaN gap, and (second case) filtered and pass-through
    sources mixed in one row."""
    steps, filt = bank
    c = rsm.resample_case(5, n_samples, steps, seed=5, passthrough=passthrough)
    assert c["gain"][0, 3] == 0 and np.isnan(c["pool"][int(c["pos"][0, 3] >> 32)])
    _check_case(c, filt, dev)


def test_both_readers_and_a_step_above_four_equal_the_restatement(dev, bank, knobs):
    """The tap loop reads a staged span from LDS, or global memory when the span does not fit (a step above 4) or
    MRMT3_RESAMPLE_LDS=0 says so: one contract."""
    steps, filt = bank
    c = rsm.resample_case(5, TILE + 37, steps, seed=6, passthrough=(2,))
    want = _restated(c, filt)
    knobs.set("MRMT3_RESAMPLE_LDS", 0)
    assert np.array_equal(_bits(_launch(c, filt, dev)), _bits(want))
    knobs.unset("MRMT3_RESAMPLE_LDS")
    assert np.array_equal(_bits(_launch(c, filt, dev)), _bits(want))
    wide = rsm.resample_case(2, TILE + 37, [5 * ONE + 12345, steps[0]], seed=7)
    wide["filt_idx"][:, 0] = 2
    got = _launch(wide, filt, dev)
    assert np.isfinite(got).all() and got[0].any() and np.array_equal(_bits(got), _bits(_restated(wide, filt)))


def test_tables_that_need_the_kernels_clamps(dev, bank):
    """begin below 0, end past the pool, a start far outside, a filter index / step / bounds that silence a source:
    the kernel computes what the contract says and reads nothing outside the pool."""
    steps, filt = bank
    rs = np.random.RandomState(3)
    pool = rs.uniform(-1, 1, 700).astype(np.float32)
    K = 8
    c = dict(pool=pool, n_samples=300, valid_samples=np.array([300, 300], np.int64),
             pos=np.tile(np.array([[(5 << 32) + 99, -(40 << 32) + 7, (650 << 32) + 3, 9 << 32, 9 << 32, 9 << 32, 9 << 32,
                                    (1 << 62) + 5]], np.int64), (2, 1)),
             begin=np.tile(np.array([[-50, -10 ** 12, 600, 0, 0, 0, 300, 0]], np.int64), (2, 1)),
             end=np.tile(np.array([[10 ** 12, 700, 750, 700, 700, 700, 300, 700]], np.int64), (2, 1)),
             step=np.tile(np.array([[steps[0], steps[1], steps[2], steps[0], 0, -steps[0], steps[0], steps[0]]], np.int64), (2, 1)),
             gain=np.ones((2, K), np.float32),
             filt_idx=np.tile(np.array([[0, 1, 2, 4, 0, 0, 0, 0]], np.int64), (2, 1)))
    c["filt_idx"][1, 3] = -7
    want = _restated(c, filt)
    got = _launch(c, filt, dev)
    assert np.isfinite(got).all() and want[0].any() and np.array_equal(_bits(got), _bits(want))
    only = dict(c, gain=c["gain"].copy())
    only["gain"][:, 3:] = 0                                                      # sources 3.. were silent or out of reach
    assert np.array_equal(_bits(_restated(only, filt)), _bits(want))


# ---- 7. pass-through equals the mix launch --------------------------------------------------------------------------

@pytest.mark.parametrize("n_samples", SIZES)
@pytest.mark.parametrize("n_src", [1, 5])
def test_pass_through_rows_are_the_stem_mix(dev, n_src, n_samples):
    from contrib import spectrograms as sp
    from mrmt3 import lib
    c = sm.stem_case(n_src, n_samples)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    shape = c["gain"].shape
    rc = dict(pool=c["pool"], pos=c["start"] << 32, begin=c["start"], end=c["end"], step=np.full(shape, ONE, np.int64),
              gain=c["gain"], filt_idx=np.full(shape, -1), valid_samples=c["valid_frames"].astype(np.int64) * HOP,
              n_samples=n_samples)
    rows = _launch(rc, np.zeros((1, 513, 2), np.float32), dev)
    want = sm.mix_rows(c["pool"], c["start"], c["end"], c["gain"], n_samples, HOP, c["valid_frames"])
    assert want.any() and np.array_equal(_bits(rows), _bits(want))
    tabs = sp.kernel_tables(sp.SpectrogramConfig(), dev)
    vf = t(c["valid_frames"], np.int32)
    for bf16 in (False, True):
        a = lib.logmel(t(rows, np.float32), tabs, valid_frames=vf, out_bf16=bf16)
        b = lib.logmel_mix(t(c["pool"], np.float32), t(c["start"], np.int64), t(c["end"], np.int64), t(c["gain"], np.float32),
                           n_samples, tabs, valid_frames=vf, out_bf16=bf16)
        assert a.dtype == (torch.bfloat16 if bf16 else torch.float32) and np.array_equal(_bits(a), _bits(b))


# ---- 8. quality of `resample` on the device -------------------------------------------------------------------------

def test_resample_is_no_worse_than_scipy_on_every_tone(dev):
    from scipy.signal import resample_poly
    from mrmt3 import lib
    from mrmt3.resample import out_length, ratio_step, resample
    step = ratio_step(Fraction(44100, 16000))
    on_dev = lambda x: resample(torch.from_numpy(x).to(dev), 44100, 16000).cpu().numpy()
    before = lib.resample_launches()
    for f in TONES:
        ref = rsm.tone_errors(lambda x: resample_poly(x.astype(np.float64), 160, 441), f, 44100, 16000, 44100)
        err = rsm.tone_errors(on_dev, f, 44100, 16000, 44100)
        print("tone %5d Hz: device %.3g, scipy %.3g" % (f, err, ref))
        assert err <= ref, (f, err, ref)
    assert lib.resample_launches() == before + len(TONES)                        # one launch each
    x = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, 5000).astype(np.float32)).to(dev)
    y = resample(x, 44100)
    assert y.shape == (out_length(5000, step),) and y.dtype == torch.float32 and resample(x, 16000) is x
    from mrmt3.resample import resample_filter
    assert np.array_equal(_bits(y), _bits(rsm.resample_1d(x.cpu().numpy(), step, resample_filter(Fraction(step, ONE)))))
    with pytest.raises(ValueError, match="ratio"):
        resample(x, 100000)
    with pytest.raises(RuntimeError, match="device"):
        resample(x.cpu(), 44100)


# ---- 9. argument errors ---------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing(dev, bank):
    import ctypes
    from mrmt3 import lib
    steps, filt = bank
    c = rsm.resample_case(2, 300, steps)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    keep = [t(c["pool"], np.float32), t(c["pos"], np.int64), t(c["begin"], np.int64), t(c["end"], np.int64),
            t(c["step"], np.int64), t(c["gain"], np.float32), t(c["filt_idx"], np.int32), t(filt, np.float32),
            torch.full((3, 300), 7.0, device=dev)]
    p = [ctypes.c_void_p(x.data_ptr()) for x in keep]
    good = [p[0], len(c["pool"]), p[1], p[2], p[3], p[4], p[5], p[6], 2, 3, 300, p[7], 4, 94, None, p[8], None]
    so = lib.load()
    before = lib.resample_launches()
    bad = [(i, None) for i in (0, 2, 3, 4, 5, 6, 7, 11, 15)]
    bad += [(8, 0), (8, 65), (13, 93), (13, 0), (13, 162), (12, -1), (1, 0), (9, 0), (10, 0), (10, -1)]
    for at, val in bad:
        args = list(good)
        args[at] = val
        assert so.mrmt3_resample_mix_fwd(*args) == 1, (at, val)                  # MRMT3_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert lib.resample_launches() == before and (keep[8] == 7.0).all()          # nothing launched, nothing written
    assert so.mrmt3_resample_mix_fwd(*good) == 0
    torch.cuda.synchronize()
    assert lib.resample_launches() == before + 1
    assert np.array_equal(_bits(keep[8]), _bits(_restated(c, filt, valid=None)))


# ---- 10. the batcher ------------------------------------------------------------------------------------------------

class _Forced(random.Random):
    """random.Random(seed) whose first randint returns `k` (the plan's shift) without consuming a draw."""

    def __init__(self, k, seed=9):
        super().__init__(seed)
        self.k, self.first = k, True

    def randint(self, a, b):
        if self.first:
            self.first = False
            return self.k
        return super().randint(a, b)


GEOM = dict(mel_length=256, event_length=256, num_rows_per_batch=2, split_frame_length=200)


def _host_pool(tr, total, offsets):
    host = np.zeros(total, np.float32)
    for off, a in zip(offsets, tr.audio):
        host[off:off + len(a)] = a
    return host


def test_batcher_builds_pitch_shifted_rows(dev):
    from contrib import spectrograms as sp
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher, pad_targets, stem_pool_layout
    from mrmt3.resample import ratio_step, resample_filter
    tr = sm.synthetic_tracks(1)[0]
    tabs = sp.kernel_tables(sp.SpectrogramConfig(), dev)
    for k in (3, -2):
        bt = StemMixBatcher(dev, pitch_shift=3, rng=_Forced(k), min_stems=2, **GEOM)
        plan = bt.plan(tr)
        assert plan.shift == k and plan.step == ratio_step(2.0 ** (k / 12.0)) and len(plan.crops.start_frame) == 2
        before, mels = lib.resample_launches(), lib.dispatch_counts()
        mel, tg = bt.build(tr, plan)
        torch.cuda.synchronize()
        took = {n: v - mels[n] for n, v in lib.dispatch_counts().items() if v != mels[n]}
        assert lib.resample_launches() == before + 1 and took == {"logmel_wave": 1}          # two launches in all
        assert mel.shape == (2, 256, 512) and mel.dtype == torch.float32
        pos, begin, end, step, gain, filt, valid, total = bt.shifted_tables(tr, plan)
        offsets, _ = stem_pool_layout([len(a) for a in tr.audio], HOP)
        rows = rsm.resample_rows(_host_pool(tr, total, offsets), pos, begin, end, step, gain, filt, 256 * HOP,
                                 resample_filter(Fraction(plan.step, ONE))[None], valid)
        assert all(rows[b].any() for b in range(2)) and np.array_equal(_bits(bt.pool(tr)), _bits(_host_pool(tr, total, offsets)))
        want = lib.logmel(torch.from_numpy(rows).to(dev), tabs, valid_frames=torch.from_numpy(plan.crops.valid_frames).to(dev))
        assert np.array_equal(_bits(mel), _bits(want))
        cpu = StemMixBatcher("cpu", pitch_shift=3, **GEOM)
        assert np.array_equal(tg.cpu().numpy(), pad_targets(cpu.row_targets(tr, plan), 256).numpy())
        t = tg.cpu().numpy()
        assert ((t == -100) | ((t >= 1) & (t < 1536))).all() and (t != -100).sum() > 10


def test_a_shift_of_zero_is_the_parent_path(dev):
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher
    tr = sm.synthetic_tracks(1)[0]
    before = lib.resample_launches()
    a = StemMixBatcher(dev, pitch_shift=3, rng=_Forced(0), **GEOM)
    b = StemMixBatcher(dev, rng=random.Random(9), **GEOM)
    plan = a.plan(tr)
    assert (plan.shift, plan.step) == (0, ONE)
    mel_a, tg_a = a.build(tr, plan)
    mel_b, tg_b = b.build(tr)
    torch.cuda.synchronize()
    assert torch.equal(mel_a, mel_b) and torch.equal(tg_a, tg_b) and lib.resample_launches() == before


def test_stems_at_their_native_rate_are_resampled_at_upload(dev):
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher, stem_pool_layout
    from mrmt3.resample import resample
    from mrmt3.stems import StemTrack
    src = sm.synthetic_tracks(1, seconds=(3.0, 2.0, 2.5))[0]
    native = StemTrack("native", src.stem_names, src.audio, src.notes, src.programs, [22050, 16000, 22050])
    down = [resample(torch.from_numpy(a).to(dev), r, 16000).cpu().numpy() for a, r in zip(src.audio, native.rates)]
    assert down[1] is not None and len(down[1]) == len(src.audio[1]) and len(down[0]) < len(src.audio[0])
    plain = StemTrack("plain", src.stem_names, down, src.notes, src.programs)
    assert native.lengths(16000) == [len(a) for a in down] and native.n_samples == plain.n_samples
    before = lib.resample_launches()
    a = StemMixBatcher(dev, pitch_shift=2, rng=_Forced(2), **GEOM)
    b = StemMixBatcher(dev, pitch_shift=2, rng=_Forced(2), **GEOM)
    pool = a.pool(native)
    torch.cuda.synchronize()
    assert lib.resample_launches() == before + 2 and a.uploads == 1              # one `resample` per stem at another rate
    offsets, total = stem_pool_layout([len(x) for x in down], HOP)
    assert pool.numel() == total and np.array_equal(_bits(pool), _bits(_host_pool(plain, total, offsets)))
    a.pool(native)
    assert lib.resample_launches() == before + 2                                  # cached: the per-step launches are the 16 kHz ones
    mel_a, tg_a = a.build(native)
    mel_b, tg_b = b.build(plain)
    assert torch.equal(mel_a, mel_b) and torch.equal(tg_a, tg_b) and mel_a.abs().sum() > 0


# ---- 11. train.py ---------------------------------------------------------------------------------------------------

TOP = """
num_epochs: 1
model_type: ${hydra:runtime.choices.model}
dataset_type: ${hydra:runtime.choices.dataset}
seed: 365
path:
event_length: 128
mel_length: 256
num_rows_per_batch: 2
split_frame_length: 300
optim:
  lr: 2e-4
  warmup_steps: 10
  num_epochs: ${num_epochs}
  num_steps_per_epoch: 100
  min_lr: 1e-4
trainer:
  log_every_n_steps: 1
dataloader:
  train:
    batch_size: 1
defaults:
  - model: MT3Net
  - dataset: Slakh
"""


def test_train_py_trains_with_pitch_shift(dev, tmp_path):
    from test_config_cpu import MODEL
    (tmp_path / "cfg" / "model").mkdir(parents=True)
    (tmp_path / "cfg" / "dataset").mkdir()
    (tmp_path / "cfg" / "config.yaml").write_text(TOP)
    (tmp_path / "cfg" / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    root = sm.write_tracks(tmp_path / "stems", sm.synthetic_tracks(2))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mr-mt3_amd")

    def run(name, *over):
        r = subprocess.run([sys.executable, os.path.join(pkg, "train.py"), "--config-dir", str(tmp_path / "cfg"),
                            "--config-name", "config", f"+stem_root={root}", "+max_steps=2",
                            f"+output_dir={tmp_path / name}"] + list(over), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        losses = [l.split()[3] for l in lines if l.startswith("step ") and " train_loss " in l]
        assert len(losses) == 2 and all(np.isfinite(float(x)) for x in losses), r.stdout
        return losses, [l for l in lines if l.startswith("resample_launches ")]

    shifted, counted = run("shift", "+stem_pitch_shift=2")
    assert len(counted) == 1 and 1 <= int(counted[0].split()[1]) <= 2, counted   # (seed 365: the first visit draws k = -1)
    plain, none = run("plain")
    zero, none0 = run("zero", "+stem_pitch_shift=0")
    assert zero == plain and not none and not none0 and shifted != plain         # the printed losses, digit for digit


# ---- 12. inference --------------------------------------------------------------------------------------------------

def test_inference_takes_audio_at_another_rate(dev):
    import inference
    from models.t5 import T5ForConditionalGeneration
    from mrmt3 import lib
    from mrmt3.resample import resample
    from mrmt3.synthetic import T5_SMALL
    audio = np.random.RandomState(42).uniform(-1, 1, 80000).astype(np.float32)       # 2.5 s at 32 kHz -> 2 segments
    model = T5ForConditionalGeneration(T5_SMALL, compute_dtype=torch.float32).load_golden().eval()
    h = inference.InferenceHandler(model=model, device=dev)
    before = lib.resample_launches()
    got, ft = h.inference(audio, batch_size=8, max_length=24, return_tokens=True, sample_rate=32000)
    assert lib.resample_launches() == before + 1
    down = resample(torch.from_numpy(audio).to(dev), 32000).cpu().numpy()
    assert len(down) == 40000
    want, ft_w = h.inference(down, batch_size=8, max_length=24, return_tokens=True)
    assert len(got) == len(want) == 1 and np.array_equal(got[0], want[0]) and np.array_equal(ft[0], ft_w[0])
    same, _ = h.inference(down, batch_size=8, max_length=24, return_tokens=True, sample_rate=16000)      # None's path
    assert np.array_equal(same[0], want[0]) and lib.resample_launches() == before + 2
    many = h.inference_many([audio, audio[:50000]], max_length=24, return_tokens=True, sample_rate=32000)
    down_b = resample(torch.from_numpy(audio[:50000]).to(dev), 32000).cpu().numpy()
    many_w = h.inference_many([down, down_b], max_length=24, return_tokens=True)
    assert all(np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1][0], b[1][0]) for a, b in zip(many, many_w))
