"""Stem-mix training batches on a real MI355X: mrmt3_logmel_mix_fwd against the contract's numpy restatement
(tests/_stem_mix.py) — bit for bit through the crops entry point, per bin against the fp64 reference of
tests/_exact_logmel.py at the kernels' existing K — then the batcher and train.py on top of it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _exact_logmel as xl
import _stem_mix as sm

pytestmark = pytest.mark.gpu

HOP = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


def _dev_tables(t, dev):
    d = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(dev) for k in ("window", "twiddle", "fb_start", "fb_cnt", "fb_w")}
    d.update(hop=t["hop"], n_mels=t["n_mels"], max_taps=t["max_taps"])
    return d


def _counted(fn, kernel):
    """fn() with the assertion that it was one launch of `kernel` ("wave" / "general")."""
    from mrmt3 import lib
    before = lib.dispatch_counts()
    out = fn()
    torch.cuda.synchronize()
    after = lib.dispatch_counts()
    took = {k: after[k] - before[k] for k in ("logmel_wave", "logmel_general")}
    assert took == {"logmel_wave": int(kernel == "wave"), "logmel_general": int(kernel == "general")}, (kernel, took)
    return out


def _bits(x):
    return x.cpu().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32).numpy()


def _mix(c, tabs, dev, vf="case", **kw):
    from mrmt3 import lib
    vf = c["valid_frames"] if isinstance(vf, str) else vf
    return lib.logmel_mix(torch.from_numpy(c["pool"]).to(dev), torch.from_numpy(c["start"]).to(dev),
                          torch.from_numpy(c["end"]).to(dev), torch.from_numpy(c["gain"]).to(dev), c["n_samples"], tabs,
                          valid_frames=None if vf is None else torch.from_numpy(vf).to(dev), **kw)


def _crops_of_rows(rows, vf, tabs, dev, **kw):
    """The host-mixed rows laid end to end as one recording, through the existing crops entry point."""
    from mrmt3 import lib
    B, n = rows.shape
    seg = torch.arange(B, dtype=torch.int64, device=dev) * n
    return lib.logmel_crops(torch.from_numpy(rows.reshape(-1)).to(dev), seg, n, tabs,
                            valid_frames=None if vf is None else torch.from_numpy(vf).to(dev), **kw)


def _host_rows(c, vf="case"):
    vf = c["valid_frames"] if isinstance(vf, str) else vf
    return sm.mix_rows(c["pool"], c["start"], c["end"], c["gain"], c["n_samples"], c["hop"], vf)


def _assert_same_bits(c, t, dev, knobs, kernels):
    rows = _host_rows(c)
    assert np.isfinite(rows).all()
    tabs = _dev_tables(t, dev)
    for kernel in kernels:
        knobs.set("MRMT3_LOGMEL", int(kernel == "wave"))
        assert xl.expected_kernel(t, int(kernel == "wave")) == kernel
        for bf16 in (False, True):
            for norm in (True, False):
                want = _counted(lambda: _crops_of_rows(rows, c["valid_frames"], tabs, dev, normalize=norm, out_bf16=bf16), kernel)
                got = _counted(lambda: _mix(c, tabs, dev, normalize=norm, out_bf16=bf16), kernel)
                assert got.shape == want.shape and got.dtype == want.dtype
                g, w = _bits(got), _bits(want)
                assert np.array_equal(g, w), "%s bf16=%s normalize=%s: %d of %d elements differ" % (kernel, bf16, norm, int((g != w).sum()), g.size)
                assert bool(torch.isfinite(got.float()).all())
                live = got[0, 0].float()
                assert float(live.max()) > float(live.min()), "a flat first frame: the mix was not read"
                F = got.shape[1]
                if c["valid_frames"][1] < F:
                    assert not bool(got[1, int(c["valid_frames"][1]):].float().any())


@pytest.mark.parametrize("n_samples", [2049, 16 * 128 + 5, 256 * 128])
@pytest.mark.parametrize("n_src", [1, 2, 5])
def test_mix_equals_the_crops_kernel_on_host_mixed_rows(dev, knobs, n_src, n_samples):
    """1. mrmt3_logmel_mix_fwd on the stems == mrmt3_logmel_crops_fwd on the rows `mix_rows` builds, bit for bit: f32 and
    bf16, wave and general kernel, normalize on and off; a stem that ends inside the crop, one that ends on a frame edge,
    a short valid_frames, a row silent past sample 0, gains 1, -0.5, 10^(+-6/20)."""
    c = sm.stem_case(n_src, n_samples)
    used = set(np.float32(c["gain"]).ravel().tolist())
    assert n_src < 2 or {np.float32(1.0), np.float32(-0.5)} <= used
    assert n_src < 5 or {float(np.float32(10 ** 0.3)), float(np.float32(10 ** -0.3))} <= used
    _assert_same_bits(c, xl.model_tables(), dev, knobs, ("wave", "general"))


def test_mix_equals_the_crops_kernel_on_a_general_only_table_set(dev, knobs):
    """... and on a table set only the general kernel takes (n_mels = 128)."""
    t = xl.tri_tables(128, 9, nan_tail=False)
    assert xl.expected_kernel(t) == "general"
    for n_src in (1, 5):
        _assert_same_bits(sm.stem_case(n_src, 16 * 128 + 5), t, dev, knobs, ("general",))


def test_one_source_at_gain_one_is_the_crops_entry_point(dev, knobs):
    """2. n_src = 1, gain 1: the same launch as mrmt3_logmel_crops_fwd on the same recording, bit for bit."""
    from mrmt3 import lib
    n, B = 16 * 128 + 5, 3
    rec = xl.noise(7, 1, 9000)[0]
    st = np.array([[0], [3001], [9000 - 700]], np.int64)               # the last crop runs past the recording's end
    vf = np.array([17, 9, 17], np.int32)
    c = dict(pool=rec, start=st, end=np.full((B, 1), len(rec), np.int64), gain=np.ones((B, 1), np.float32), valid_frames=vf,
             n_samples=n, hop=HOP)
    tabs = _dev_tables(xl.model_tables(), dev)
    for kernel in ("wave", "general"):
        knobs.set("MRMT3_LOGMEL", int(kernel == "wave"))
        for bf16 in (False, True):
            want = _counted(lambda: lib.logmel_crops(torch.from_numpy(rec).to(dev), torch.from_numpy(st[:, 0].copy()).to(dev), n, tabs,
                                                     valid_frames=torch.from_numpy(vf).to(dev), out_bf16=bf16), kernel)
            got = _counted(lambda: _mix(c, tabs, dev, out_bf16=bf16), kernel)
            assert np.array_equal(_bits(got), _bits(want)), (kernel, bf16)


@pytest.mark.parametrize("kind", ["noise", "tone"])
def test_mixed_rows_meet_the_fp64_bound_of_the_frontend(dev, knobs, kind):
    """3. The mix is exact by contract, so the per-bin bound of tests/_exact_logmel.py holds on the host-mixed rows with the
    kernels' K_WAVE / K_GENERAL unchanged; the noise case accepts no floor-rule element."""
    n = xl.N_A
    if kind == "noise":
        c = sm.stem_case(4, n, seed=11)                              # rows 0 and 1 (row 2 is silence: all floor, no noise case)
        c = {k: (v[:2] if k in ("start", "end", "gain") else v) for k, v in c.items()}
        t = xl.model_tables()
    else:                                                           # on-bin cosines under a window of ones, one per source
        k0s = (15, 64, 513)
        tones = xl.on_bin_tones(k0s * 2, n)                         # [6, n]: rows 0-1 x 3 sources
        pool = tones.reshape(-1)
        start = (np.arange(6, dtype=np.int64) * n).reshape(2, 3)
        c = dict(pool=pool, start=start, end=start + n, gain=np.array([[1, -0.5, 10 ** 0.3], [10 ** -0.3, 1, 0.75]], np.float32),
                 valid_frames=None, n_samples=n, hop=HOP)
        t = xl.identity_tables(0, 512, np.ones(xl.FFT_N, np.float32))
    rows = _host_rows(c, vf=None)
    case = xl.case("mix_" + kind, rows, t, "wave", noise_case=(kind == "noise"), allow_floor=(kind == "tone"))
    ref = xl.reference(case)
    tabs = _dev_tables(t, dev)
    for kernel in ("wave", "general"):
        knobs.set("MRMT3_LOGMEL", int(kernel == "wave"))
        got = _counted(lambda: _mix(c, tabs, dev, vf=None, normalize=False), kernel).cpu().numpy()
        ratio, n_floor = xl.check(case["name"], got, ref, case, kernel)
        print("%s [%s]: ratio %.3f, floor-accepted %d" % (case["name"], kernel, ratio, n_floor))
        assert kind != "noise" or n_floor == 0


def test_nothing_outside_the_tables_is_read(dev, knobs):
    """4. The pool is a view in the middle of one larger NaN-filled allocation.  Gain-0 sources point into the NaN (before
    and behind the pool), one source's end lies past pool_samples (clamped), one starts below 0 (silent): the output is
    finite and equals the restatement under the clamping rules."""
    n, P, G = 16 * 128 + 5, 6000, 5001
    big = torch.full((G + P + G,), float("nan"), device=dev)
    rs = np.random.RandomState(5)
    host = rs.uniform(-1, 1, P).astype(np.float32)
    big[G:G + P] = torch.from_numpy(host).to(dev)
    pool = big[G:G + P]
    assert pool.is_contiguous() and pool.data_ptr() == big.data_ptr() + 4 * G
    start = np.array([[100, -300, P + 50, P - 1000], [-1, 2000, -G + 3, 0], [P - 1, P, 10 ** 12, -10 ** 12]], np.int64)
    end = np.array([[3000, 500, P + 900, P + 500], [4000, 2700, 100, 1], [P + 10 ** 9, P + 5, 10 ** 13, 5]], np.int64)
    gain = np.array([[1, 0, 0, -0.5], [2, 0.75, 0, 1], [1, 3, 0, 1]], np.float32)
    #  row 0: plain | gain 0 before the pool | gain 0 behind the pool | end > pool_samples: reads up to P
    #  row 1: start < 0: silent | ends inside the crop | gain 0 in the NaN before the pool | one sample
    #  row 2: the pool's last sample, end far past it | start == pool_samples: silent | gain 0, absurd | start < 0: silent
    c = dict(pool=host, start=start, end=end, gain=gain, valid_frames=None, n_samples=n, hop=HOP)
    rows = _host_rows(c)
    assert np.array_equal(rows[0, :1000], (host[100:1100] + (np.float32(-0.5) * host[P - 1000:]).astype(np.float32)))
    assert np.array_equal(rows[1, :700], (np.float32(0.75) * host[2000:2700]).astype(np.float32) + np.r_[host[0], np.zeros(699, np.float32)])
    assert rows[2, 0] == host[P - 1] and not rows[2, 1:].any()
    from mrmt3 import lib
    tabs = _dev_tables(xl.model_tables(), dev)
    dt = lambda a: torch.from_numpy(a).to(dev)
    for kernel in ("wave", "general"):
        knobs.set("MRMT3_LOGMEL", int(kernel == "wave"))
        got = _counted(lambda: lib.logmel_mix(pool, dt(start), dt(end), dt(gain), n, tabs), kernel)
        assert bool(torch.isfinite(got).all()), kernel + ": NaN from outside the tables reached the output"
        want = _crops_of_rows(rows, None, tabs, dev)
        assert np.array_equal(_bits(got), _bits(want)), kernel
    assert bool(torch.isnan(big[:G]).all()) and bool(torch.isnan(big[G + P:]).all())


def test_batcher_end_to_end(dev):
    """5. StemMixBatcher.build: mel bit-equal to logmel_segments of the host-mixed rows, targets equal to the CPU path, a
    finite training loss, and an LRU device cache that drops a track without changing a result."""
    import random
    from contrib import spectrograms as sp
    from mrmt3.batching import StemMixBatcher, pad_targets, stem_pool_layout
    from mrmt3.trainer import Trainer
    from test_train_infer_gpu import _model
    tracks = sm.synthetic_tracks(2)
    geom = dict(mel_length=256, event_length=256, num_rows_per_batch=2, split_frame_length=300)
    one_track = stem_pool_layout([len(a) for a in tracks[0].audio], HOP)[1] * 4
    bt = StemMixBatcher(dev, rng=random.Random(3), min_stems=2, cache_bytes=one_track + 4096, **geom)
    results = []
    for tr in tracks:
        plan = bt.plan(tr)
        assert plan.keep.sum(1).min() >= 2 and len(plan.crops.start_frame) == 2
        mel, tg = bt.build(tr, plan)
        assert mel.shape == (2, 256, 512) and mel.dtype == torch.float32 and tg.shape == (2, 256) and tg.dtype == torch.int64
        start, end, gain, total = bt.tables(tr, plan)
        offsets, _ = stem_pool_layout([len(a) for a in tr.audio], HOP)
        host = np.zeros(total, np.float32)
        for off, a in zip(offsets, tr.audio):
            host[off:off + len(a)] = a
        rows = sm.mix_rows(host, start * HOP, end, gain, 256 * HOP, HOP, plan.crops.valid_frames)
        assert all(rows[b].any() for b in range(2))
        want = sp.logmel_segments(torch.from_numpy(rows).to(dev), valid_frames=torch.from_numpy(plan.crops.valid_frames).to(dev))
        assert np.array_equal(_bits(mel), _bits(want))
        assert np.array_equal(tg.cpu().numpy(), pad_targets(StemMixBatcher("cpu", **geom).row_targets(tr, plan), 256).numpy())
        t = tg.cpu().numpy()
        assert ((t == -100) | ((t >= 1) & (t < 1536))).all() and (t != -100).sum() > 10
        results.append((plan, mel, tg))
    # the cache holds one track: the second upload dropped the first; building it again uploads again, same bits
    assert bt.uploads == 2 and bt.cached_tracks() == [tracks[1].name]
    mel0, tg0 = bt.build(tracks[0], results[0][0])
    assert bt.uploads == 3 and bt.cached_tracks() == [tracks[0].name]
    assert torch.equal(mel0, results[0][1]) and torch.equal(tg0, results[0][2])
    bt.build(tracks[0], results[0][0])
    assert bt.uploads == 3                                            # a hit
    roomy = StemMixBatcher(dev, is_deterministic=True, **geom)
    for tr in tracks:
        roomy.build(tr)
    assert roomy.uploads == 2 and roomy.cached_tracks() == [t.name for t in tracks]
    m = _model("t5", dev)
    trn = Trainer(m, lr=1e-3)
    loss = trn.train_step(results[0][1], results[0][2]).item()
    assert np.isfinite(loss) and loss > 0
    trn.close()


def test_train_py_trains_from_a_stem_folder(dev, tmp_path):
    """6. `train.py +stem_root=<dir> +max_steps=2` in a child process: the step lines, last.pt, and with +stem_val_root the
    val_loss line."""
    from test_config_cpu import MODEL
    top = """
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
    (tmp_path / "cfg" / "model").mkdir(parents=True)
    (tmp_path / "cfg" / "dataset").mkdir()
    (tmp_path / "cfg" / "config.yaml").write_text(top)
    (tmp_path / "cfg" / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    root = sm.write_tracks(tmp_path / "stems", sm.synthetic_tracks(2))
    val = sm.write_tracks(tmp_path / "val", sm.synthetic_tracks(1, seed=9))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mr-mt3_amd")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(pkg, "train.py"), "--config-dir", str(tmp_path / "cfg"), "--config-name", "config",
                        f"+stem_root={root}", f"+stem_val_root={val}", "+max_steps=2", f"+output_dir={out}"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert any(l.startswith("step 0 train_loss ") for l in lines) and any(l.startswith("step 1 train_loss ") for l in lines), r.stdout
    vals = [l for l in lines if " val_loss " in l]
    assert vals and np.isfinite(float(vals[-1].split()[-1])), r.stdout
    ckpt = out / "MT3Net_Slakh" / "version_0" / "checkpoints"
    assert (ckpt / "last.pt").exists() and torch.load(ckpt / "last.ckpt", weights_only=False)["global_step"] == 2
