"""End-to-end checks of the MI355X trainer and inference harness on a real GPU."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(variant, dev, **cfg_over):
    from mrmt3.synthetic import T5_SMALL
    cfg = dict(T5_SMALL, **cfg_over)
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        return T5ForConditionalGeneration(cfg).load_golden().to(dev)
    from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
    return T5SegMemV2WithPrev(cfg, 1, 64).load_golden().to(dev)


def test_fused_ce_step_equals_torch_ce_step(dev):
    """Trainer path (fused CE kernel, grads into the flat buffer) == drop-in path (torch CE on the
    returned logits + loss.backward()) on the same batch, dropout off."""
    from mrmt3.synthetic import synth_mel, synth_labels
    from mrmt3.trainer import Trainer
    mel = torch.from_numpy(synth_mel(2)).to(dev)
    lab = torch.from_numpy(synth_labels(2, 256, full=False, seed=5, mean_len=100)).to(dev)
    m1 = _model("t5", dev, dropout_rate=0.0)
    m1.train()
    out = m1(inputs=mel, labels=lab)
    loss1 = torch.nn.functional.cross_entropy(out.view(-1, 1536), lab.view(-1), ignore_index=-100)
    loss1.backward()
    g1 = m1.flat.G.clone()
    m2 = _model("t5", dev, dropout_rate=0.0)
    tr = Trainer(m2, lr=0.0)
    p_before = m2.flat.P.clone()
    loss2 = tr.train_step(mel, lab)
    assert abs(loss1.item() - loss2.item()) < 2e-4
    # dlogits are rounded to bf16 in the fused path, f32->bf16 cast in the other: same values up to rounding
    rel = ((m2.flat.G - g1).norm() / g1.norm()).item()
    assert rel < 2e-2, rel
    assert torch.equal(m2.flat.P, p_before * (1.0 - 0.0))          # lr = 0: AdamW leaves the weights alone


@pytest.mark.parametrize("variant", ["t5", "with_prev"])
def test_trainer_learns_from_audio(dev, variant):
    """Audio -> log-mel -> fwd/bwd -> AdamW for a few steps on one fixed batch: the loss must fall."""
    from mrmt3.synthetic import synth_audio, synth_labels
    from mrmt3.trainer import Trainer
    m = _model(variant, dev)
    tr = Trainer(m, lr=1e-3)
    audio = torch.from_numpy(synth_audio(4)).to(dev)
    lab = torch.from_numpy(synth_labels(4, 256, full=False, seed=9, mean_len=120)).to(dev)
    prev = torch.from_numpy(synth_labels(4, 256, full=False, seed=10, mean_len=120)).to(dev) if variant != "t5" else None
    losses = [tr.train_step(audio, lab, None if prev is None else prev.clone(), audio=True).item() for _ in range(8)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.3, losses
    assert int(tr.step_dev.item()) == 8
    ev = tr.eval_loss(audio, lab, None if prev is None else prev.clone(), audio=True).item()
    assert np.isfinite(ev)


def test_weighted_loss_trainer_matches_oracle(dev):
    from mrmt3.synthetic import synth_mel, synth_labels, T5_SMALL, golden_weights
    from mrmt3.trainer import Trainer
    from oracle import t5_ref
    mel = torch.from_numpy(synth_mel(1))
    lab = torch.from_numpy(synth_labels(1, 256, full=False, seed=3, mean_len=150))
    sd = {k: torch.from_numpy(v) for k, v in golden_weights(T5_SMALL).items()}
    with torch.no_grad():
        ref = t5_ref.weighted_ce_loss(t5_ref.forward_logits(sd, T5_SMALL, mel, lab), lab).item()
    m = _model("t5", dev, dropout_rate=0.0)
    tr = Trainer(m, lr=0.0, weighted_loss=True)
    got = tr.eval_loss(mel.to(dev), lab.to(dev)).item()
    assert abs(got - ref) < 2e-3


def test_inference_handler_matches_oracle_pipeline(dev):
    """audio -> InferenceHandler (one log-mel launch for all segments, KV-cached decode) vs the
    oracle's restatement of inference.py (fp32, short max_length)."""
    import inference
    from models.t5 import T5ForConditionalGeneration
    from mrmt3.synthetic import T5_SMALL, golden_weights
    from oracle import logmel_ref, t5_ref
    audio = np.random.RandomState(42).uniform(-1, 1, 40000).astype(np.float32)       # 313 frames -> 2 segments
    model = T5ForConditionalGeneration(T5_SMALL, compute_dtype=torch.float32).load_golden().eval()
    h = inference.InferenceHandler(model=model, device=dev)
    mel_dev, ft = h._preprocess(audio)
    mel_ref, ft_ref, pads = logmel_ref.preprocess(audio)
    assert pads == [256, 57] and np.array_equal(ft, ft_ref)
    np.testing.assert_allclose(mel_dev.cpu().numpy(), mel_ref, atol=1e-4, rtol=0)
    assert (mel_dev[1, 57:] == 0).all()
    results, _ = h.inference(audio, batch_size=8, max_length=24, return_tokens=True)
    sd = {k: torch.from_numpy(v) for k, v in golden_weights(T5_SMALL).items()}
    with torch.no_grad():
        ref_ids = t5_ref.generate_t5(sd, T5_SMALL, torch.from_numpy(mel_ref.astype(np.float32)), max_length=24)
    np.testing.assert_array_equal(results[0], logmel_ref.postprocess_batch(ref_ids.numpy()))
    # audio -> MIDI file end to end (random weights: the notes are meaningless, the plumbing is what is checked)
    import os
    import tempfile
    from oracle import notes_ref
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out", "song.mid")
        ns = h.inference(audio, outpath=out, batch_size=8, max_length=24)
        assert open(out, "rb").read(4) == b"MThd"
    ref_notes, _, _ = notes_ref.to_event(results, [ft])
    assert [[n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument] for n in ns.notes] == ref_notes


def test_checkpoint_resume_continues_the_same_trajectory(dev, tmp_path):
    """save -> new process-equivalent (fresh model + trainer) -> resume: weights, AdamW moments, step
    counter, LR schedule position and dropout stream all continue; the next step lands on bit-identical
    weights (no float atomics feed the gradients: sorted embedding gradient, ordered split-K and norm-weight
    reductions)."""
    from mrmt3 import checkpoint as ck
    from mrmt3.synthetic import synth_audio, synth_labels
    from mrmt3.trainer import Trainer
    from utils import cosine_warmup_lambda
    lam = cosine_warmup_lambda(4, 100, min_lr=1e-4)
    audio = [torch.from_numpy(synth_audio(2, seed=s)).to(dev) for s in (1, 2, 3)]
    labs = [torch.from_numpy(synth_labels(2, 256, full=False, seed=s, mean_len=100)).to(dev) for s in (4, 5, 6)]
    m = _model("t5", dev)
    tr = Trainer(m, lr=1e-3, lr_lambda=lam)
    for i in range(2):
        tr.train_step(audio[i], labs[i], audio=True)
    path = str(tmp_path / "last.ckpt")
    tr.save_checkpoint(path)
    M2, V2 = m.flat.M.clone(), m.flat.V.clone()
    loss_a = tr.train_step(audio[2], labs[2], audio=True).item()
    P_a = m.flat.P.clone()

    blob = torch.load(path, weights_only=False)
    assert blob["global_step"] == 2 and len(blob["optimizer_states"][0]["state"]) == 189
    assert all(k.startswith("model.") for k in blob["state_dict"])

    m2 = _model("t5", dev)
    with torch.no_grad():
        m2.flat.P.add_(0.01)                      # make sure the weights really come from the file
    tr2 = Trainer(m2, lr=1e-3, lr_lambda=lam)
    assert tr2.resume(path) == 2 and int(tr2.step_dev.item()) == 2
    assert torch.equal(m2.flat.M, M2) and torch.equal(m2.flat.V, V2)
    loss_b = tr2.train_step(audio[2], labs[2], audio=True).item()
    assert abs(loss_a - loss_b) < 1e-5, (loss_a, loss_b)
    assert torch.equal(m2.flat.P, P_a)
    assert abs(tr2.lr_dev.item() - tr.lr_dev.item()) < 1e-12

    # the optimizer state is a valid torch.optim.AdamW state for the reference's parameter order
    order = ck.reference_parameter_order(m.cfg, 0)
    opt = torch.optim.AdamW([m2._views[k] for k in order], lr=1e-3)
    opt.load_state_dict(blob["optimizer_states"][0])
    assert float(opt.state[m2._views[order[0]]]["step"]) == 2.0

    # bare export (train.py:105-116)
    tr2.save_checkpoint(str(tmp_path / "last.pt"))
    sd = torch.load(tmp_path / "last.pt")
    assert "proj.weight" in sd and not any(k.startswith("model.") for k in sd)


def test_train_py_resume_and_export(dev, tmp_path):
    """train.py end to end on a reference-shaped config: 2 steps, export, then `path=...last.ckpt` resumes."""
    import train
    top = """
num_epochs: 1
model_type: ${hydra:runtime.choices.model}
dataset_type: ${hydra:runtime.choices.dataset}
seed: 365
path:
event_length: 128
mel_length: 256
num_rows_per_batch: 2
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
    from test_config_cpu import MODEL
    (tmp_path / "cfg" / "model").mkdir(parents=True)
    (tmp_path / "cfg" / "dataset").mkdir()
    (tmp_path / "cfg" / "config.yaml").write_text(top)
    (tmp_path / "cfg" / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    out = tmp_path / "out"
    base = ["--config-dir", str(tmp_path / "cfg"), "--config-name", "config", "+synthetic=True"]
    train.main(base + ["+max_steps=2", f"+output_dir={out}"])
    ckpt = out / "MT3Net_Slakh" / "version_0" / "checkpoints" / "last.ckpt"
    assert ckpt.exists() and (ckpt.parent / "last.pt").exists()
    assert torch.load(ckpt, weights_only=False)["global_step"] == 2
    out2 = tmp_path / "out2"
    train.main(base + ["+max_steps=1", f"+output_dir={out2}", f"path={ckpt}"])
    assert torch.load(out2 / "MT3Net_Slakh" / "version_0" / "checkpoints" / "last.ckpt", weights_only=False)["global_step"] == 3
    with pytest.raises(ValueError):
        train.main(base + ["+max_steps=1", f"+output_dir={out2}", "path=weights.bin"])
    # without +synthetic the configured dataset is instantiated (train.py:48-59) ...
    import sys
    (tmp_path / "toyset.py").write_text(
        "import numpy as np, torch\n"
        "from torch.utils.data import Dataset\n"
        "class Toy(Dataset):\n"
        "    def __init__(self, mel_length, n): self.L, self.n = mel_length, n\n"
        "    def __len__(self): return self.n\n"
        "    def __getitem__(self, i):\n"
        "        rs = np.random.RandomState(i)\n"
        "        return (torch.from_numpy(rs.rand(2, self.L, 512).astype('float32')),\n"
        "                torch.from_numpy(rs.randint(3, 1000, size=(2, 128)).astype('int64')))\n"
        "def collate(batch):\n"
        "    return torch.cat([b[0] for b in batch]), torch.cat([b[1] for b in batch])\n")
    sys.path.insert(0, str(tmp_path))
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text(
        "train:\n  _target_: toyset.Toy\n  mel_length: ${mel_length}\n  n: 3\n"
        "val:\n  _target_: toyset.Toy\n  mel_length: ${mel_length}\n  n: 1\n"
        "collate_fn: toyset.collate\n")
    (tmp_path / "cfg" / "config.yaml").write_text(top.replace("    batch_size: 1\n", "    batch_size: 1\n  val:\n    batch_size: 1\n"))
    real = ["--config-dir", str(tmp_path / "cfg"), "--config-name", "config"]
    out3 = tmp_path / "out3"
    train.main(real + [f"+output_dir={out3}"])            # one epoch of 3 batches + validation
    assert torch.load(out3 / "MT3Net_Slakh" / "version_0" / "checkpoints" / "last.ckpt", weights_only=False)["global_step"] == 3
    # ... and a dataset package that cannot be imported stops the run instead of training on synthetic data
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text(
        "train:\n  _target_: dataset_not_installed.Slakh\nval:\n  _target_: dataset_not_installed.Slakh\n"
        "collate_fn: dataset_not_installed.collate\n")
    with pytest.raises(RuntimeError, match="synthetic"):
        train.main(real + [f"+output_dir={out3}"])


def test_rows_from_a_recording_feed_the_trainer(dev):
    """Recording + its notes -> Tokenizer (targets) + DeviceBatcher (crops read on the GPU) -> train_step."""
    import random
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.batching import DeviceBatcher
    from mrmt3.tokenizer import Tokenizer
    from mrmt3.trainer import Trainer
    rs = np.random.RandomState(3)
    seconds = 40.0
    song = rs.uniform(-0.5, 0.5, size=int(seconds * 16000)).astype(np.float32)
    notes = []
    for _ in range(400):
        s = float(rs.uniform(0, seconds - 1))
        notes.append(Note(s, s + float(rs.uniform(0.05, 0.8)), int(rs.randint(30, 90)), 90, int(rs.choice([0, 33])), False))
    tk = Tokenizer()
    feats = tk.tokenize(NoteSequence(notes, seconds), len(song))
    bt = DeviceBatcher(dev, mel_length=256, event_length=256, num_rows_per_batch=4, split_frame_length=1000,
                       out_bf16=True, rng=random.Random(1))
    audio = bt.upload(song)
    mel, targets = bt.build(audio, tk.targets_for_crop(feats))
    assert mel.shape == (4, 256, 512) and mel.dtype == torch.bfloat16 and targets.shape == (4, 256)
    t = targets.cpu().numpy()
    assert ((t == -100) | ((t >= 1) & (t < 1536))).all() and (t != -100).sum() > 40
    first_pad = [(row == -100).argmax() if (row == -100).any() else 256 for row in t]
    assert all(row[p - 1] == 1 for row, p in zip(t, first_pad) if p < 256)          # EOS closes every short row
    m = _model("t5", dev)
    tr = Trainer(m, lr=1e-3)
    losses = [tr.train_step(mel, targets).item() for _ in range(10)]
    assert all(np.isfinite(losses)) and min(losses[-3:]) < losses[0], losses


def test_test_py_transcribes_a_directory_and_scores_it(dev, tmp_path):
    """test.py end to end on a Slakh-shaped tree: WAV files -> MIDI files -> evaluate_main, with an MR-MT3 model
    (recordings decoded in lockstep) loaded from a bare state-dict file."""
    import importlib
    from contrib import audio_io, midi_io
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.synthetic import T5_SMALL, golden_weights
    from test_config_cpu import MODEL
    drv = importlib.import_module("test")                # mr-mt3_amd/test.py (the drop-in root precedes the stdlib on sys.path)
    assert hasattr(drv, "get_scores")
    top = """
model_type: ${hydra:runtime.choices.model}
dataset_type: ${hydra:runtime.choices.dataset}
seed: 365
path:
model_segmem_length: 64
optim:
  lr: 2e-4
  warmup_steps: 10
  num_epochs: 1
  num_steps_per_epoch: 100
  min_lr: 1e-4
eval:
  audio_dir:
  midi_dir:
  eval_dataset: Slakh
  exp_tag_name: run1
  batch_size: 8
  contiguous_inference: False
  eval_first_n_examples:
  load_weights_strict:
defaults:
  - model: MT3NetSegMemV2WithPrev
  - dataset: Slakh
"""
    cfgd = tmp_path / "cfg"
    (cfgd / "model").mkdir(parents=True)
    (cfgd / "dataset").mkdir()
    (cfgd / "config.yaml").write_text(top)
    seg = "segmem_num_layers: 1\n  segmem_length: ${model_segmem_length}"
    (cfgd / "model" / "MT3NetSegMemV2WithPrev.yaml").write_text(
        MODEL % ("mt3_net_segmem_v2_with_prev.MT3NetSegMemV2WithPrev", seg))
    (cfgd / "dataset" / "Slakh.yaml").write_text("test:\n  root_dir: unused\n")
    # weights: the golden recipe with EOS made competitive so every segment ends early
    w = golden_weights(T5_SMALL, 1)
    w["lm_head.weight"] = w["lm_head.weight"].copy()
    w["lm_head.weight"][1] *= 3.0
    torch.save({k: torch.from_numpy(v) for k, v in w.items()}, tmp_path / "weights.pt")
    rs = np.random.RandomState(0)
    gt = NoteSequence([Note(0.5, 1.0, 60, 90, 0, False, 0), Note(1.0, 1.4, 64, 90, 33, False, 1)], 1.4)
    for k, secs in enumerate((3.0, 5.0, 2.2)):
        d = tmp_path / "audio" / f"Track{k:02d}"
        d.mkdir(parents=True)
        audio_io.write_wav(str(d / "mix_16k.wav"), rs.uniform(-0.3, 0.3, int(secs * 16000)))
        g = tmp_path / "gt" / f"Track{k:02d}"
        g.mkdir(parents=True)
        midi_io.note_sequence_to_midi_file(gt, str(g / "all_src_v2.mid"))
    out = tmp_path / "out"
    scores = drv.main(["--config-dir", str(cfgd), "--config-name", "config", f"path={tmp_path / 'weights.pt'}",
                       f"eval.audio_dir={tmp_path}/audio/*/mix_16k.wav", f"eval.midi_dir={tmp_path}/gt",
                       f"+output_dir={out}", "+eval.songs_per_batch=2"])
    for k in range(3):
        assert (out / "run1" / f"Track{k:02d}" / "mix.mid").exists()
        midi_io.read_midi(str(out / "run1" / f"Track{k:02d}" / "mix.mid"))          # a well-formed MIDI file
    assert "Onset F1" in scores and "Onset + program F1 (midi_class)" in scores
    assert all(0.0 <= v <= 1.0 for v in scores.values() if not isinstance(v, dict))


def test_full_benchmark_batch_gradient_is_the_mean_of_its_halves(dev):
    """BASELINE configs[1] at full size (64 segments x 1024 tokens, dropout off): the gradient of the batch equals
    the mean of the gradients of its two halves (a size-independent property of the whole fwd+bwd path), and the
    step is bitwise reproducible."""
    from mrmt3.synthetic import synth_audio, synth_labels
    from mrmt3.trainer import Trainer
    m = _model("t5", dev, dropout_rate=0.0)
    tr = Trainer(m, lr=0.0)
    audio = torch.from_numpy(synth_audio(64, seed=8)).to(dev)
    lab = torch.from_numpy(synth_labels(64, seed=9)).to(dev)
    loss = tr.train_step(audio, lab, audio=True).item()
    g_all = m.flat.G.clone()
    tr.train_step(audio, lab, audio=True)
    assert torch.equal(m.flat.G, g_all)
    la = tr.train_step(audio[:32], lab[:32], audio=True).item()
    g_a = m.flat.G.clone()
    lb = tr.train_step(audio[32:], lab[32:], audio=True).item()
    g_b = m.flat.G.clone()
    assert abs(loss - (la + lb) / 2) < 2e-5
    rel = ((g_all - (g_a + g_b) / 2).norm() / g_all.norm()).item()
    assert rel < 3e-3, rel


def test_bf16_shadows_follow_torch_optimizer_and_load_state_dict(dev):
    """after `.to(device)` torch.optim.AdamW / load_state_dict write through Parameters whose
    version counters are not P's; the bf16 shadow (and transposed dgrad copy) must still be rebuilt."""
    from mrmt3.synthetic import synth_mel, synth_labels
    mel = torch.from_numpy(synth_mel(2)).to(dev)
    lab = torch.from_numpy(synth_labels(2, 128, full=False, seed=5, mean_len=60)).to(dev)
    m = _model("t5", dev, dropout_rate=0.0)
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    for _ in range(2):
        out = m(inputs=mel, labels=lab)
        loss = torch.nn.functional.cross_entropy(out.view(-1, 1536), lab.view(-1), ignore_index=-100)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.step()
    m.engine.prepare(True)
    assert torch.equal(m.flat.S, m.flat.P.bfloat16())
    o, r, c = m.flat.groups["lm_head"]
    assert torch.equal(m.flat.WT("lm_head"), m.flat.S[o:o + r * c].view(r, c).t().contiguous())
    # forward, load other weights, forward again: the logits must change
    m.eval()
    with torch.no_grad():
        a = m(inputs=mel, labels=lab).clone()
        other = {k: (v * 0.5 if v.dim() == 2 else v) for k, v in m.state_dict().items()}
        m.load_state_dict(other)
        b = m(inputs=mel, labels=lab)
    assert (a - b).abs().max().item() > 1e-2
    assert torch.equal(m.flat.S, m.flat.P.bfloat16())


@pytest.mark.parametrize("variant", ["t5", "with_prev"])
def test_bf16_training_trajectory_tracks_the_fp32_oracle(dev, variant):
    """16 optimizer steps on one fixed batch, dropout off: the bf16 HIP trainer (graph replay from step 3 on) against
    the fp32 CPU oracle driven by torch.optim.AdamW with the same hyper-parameters (tasks/mt3_net.py:58-68: AdamW over
    all parameters; torch defaults betas (0.9, 0.999), eps 1e-8, weight_decay 0.01).  The two loss curves stay together
    step by step — a wrong moment update, a dropped gradient term or drifting bf16 shadows shows up as a growing gap —
    and the weights end up where the oracle's do."""
    from mrmt3.synthetic import T5_SMALL, golden_weights, synth_mel, synth_labels
    from mrmt3.trainer import Trainer
    from oracle import t5_ref
    torch.set_num_threads(8)
    B, steps, lr = 2, 16, 1e-4
    cfg = dict(T5_SMALL, dropout_rate=0.0)
    mel = torch.from_numpy(synth_mel(B))
    lab = torch.from_numpy(synth_labels(B, 256, full=False, seed=21, mean_len=120))
    prev = torch.from_numpy(synth_labels(B, 256, full=False, seed=22, mean_len=120)) if variant != "t5" else None
    ovar = "t5" if variant == "t5" else "segmem_v2_with_prev"
    sd = {k: torch.from_numpy(v.copy()) for k, v in golden_weights(T5_SMALL, 0 if variant == "t5" else 1).items()}
    params = [v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "inv_freq" not in k]
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    ref_losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        logits = t5_ref.forward_logits(sd, cfg, mel, lab, variant=ovar, targets_prev=None if prev is None else prev.clone())
        loss = t5_ref.ce_loss(logits, lab)
        loss.backward()
        opt.step()
        ref_losses.append(loss.item())
    m = _model(variant, dev, dropout_rate=0.0)
    tr = Trainer(m, lr=lr)
    mel_d, lab_d = mel.to(dev), lab.to(dev)
    losses = [tr.train_step(mel_d, lab_d, None if prev is None else prev.clone().to(dev)).item() for _ in range(steps)]
    assert tr.graph_captured or not tr.use_graph
    gaps = [abs(a - b) for a, b in zip(losses, ref_losses)]
    print(variant, "loss oracle/hip:", ["%.4f/%.4f" % (a, b) for a, b in zip(ref_losses, losses)])
    assert ref_losses[-1] < ref_losses[0] - 1.0, ref_losses                   # the batch is being learnt
    assert gaps[0] < 1e-3 and max(gaps) < 1.2e-2, gaps      # measured: <= 6.6e-3 (t5), 6.6e-3 (with_prev) while the loss falls 7.8 -> 0.1
    # weights: compare the update (what 16 steps changed), tensor by tensor
    init = golden_weights(T5_SMALL, 0 if variant == "t5" else 1)
    worst = 0.0
    for k, ref in sd.items():
        if not ref.requires_grad or ref.grad is None:
            continue
        d_ref = ref.detach() - torch.from_numpy(init[k])
        d_hip = m.state_dict()[k].float().cpu() - torch.from_numpy(init[k])
        if d_ref.norm() < 1e-6:
            continue
        cos = torch.nn.functional.cosine_similarity(d_hip.flatten(), d_ref.flatten(), dim=0).item()
        worst = max(worst, 1.0 - cos)
        assert cos > 0.99, (k, cos)                                  # measured worst 0.9976
    print(variant, "worst 1 - cos(update):", worst)


def test_step_gradients_do_not_depend_on_the_launch_structure(dev, knobs):
    """One backward, three ways of launching it: (a) the default (weight gradients grouped into one launch, wi projection
    fused with the gated GELU, cross k|v of all layers from one projection), (b) the wi projection and the GELU as two
    kernels — bit-identical by construction, so the whole gradient must be — and (c) one launch per weight gradient —
    a different f32 summation order over the token rows, so equal to rounding noise only.  (c) is the fallback of the
    grouped launch: its counters show that mrmt3_gemm_tn really ran there."""
    from mrmt3 import lib
    from mrmt3.synthetic import synth_mel, synth_labels
    from mrmt3.trainer import Trainer
    mel = torch.from_numpy(synth_mel(8)).to(dev)
    lab = torch.from_numpy(synth_labels(8, 1024, full=True, seed=3)).to(dev)

    def grads(**env):
        for k, v in env.items():
            knobs.set(k, v)
        m = _model("t5", dev, dropout_rate=0.1)
        tr = Trainer(m, lr=0.0, graph=False)
        lib.dispatch_counts(reset=True)
        loss = tr.train_step(mel, lab).item()
        torch.cuda.synchronize()
        tr.launches = lib.dispatch_counts()
        for k in env:
            knobs.unset(k)
        return loss, m.flat.G.clone(), tr

    l0, g0, tr0 = grads()
    assert tr0.launches["tn_group"] > 0
    assert tr0.engine.tn_group is not None and tr0.engine.tn_group.last_info.n_items > 0          # the grouped launch ran
    l1, g1, _ = grads(MRMT3_GEGLU_FUSED="0")
    assert abs(l0 - l1) < 2e-6 and torch.equal(g0, g1)
    l2, g2, tr2 = grads(MRMT3_TN_GROUP="0")
    assert tr2.engine.tn_group is None
    assert tr2.launches["tn8"] + tr2.launches["tn_tile"] > 0 and tr2.launches["tn_group"] == 0, tr2.launches
    rel = ((g0 - g2).norm() / g2.norm()).item()
    assert abs(l0 - l2) < 2e-6 and rel < 2e-6, rel
    assert (g0 - g2).abs().max().item() < 1e-5 * g2.abs().max().item() + 1e-7


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(dev, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps, prints the headline line and nothing of what
    `--full` adds; `--dump-outputs DIR` writes the last timed step's loss and fixed samples of the updated parameters and
    of the gradient as float32 .npy files, 64 MB at most."""
    import json
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "outputs"
    r = subprocess.run([_sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-500:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "segments/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["ms_per_step"] > 0 and abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for k in ("roofline", "train_b12", "train_mrmt3", "train_mrmt3_b12", "train_long_context", "inference", "cpu_baseline"):
        assert k not in d, k
    names = sorted(os.listdir(out))
    assert names == ["grads_sample.npy", "loss.npy", "params_sample.npy"], names
    assert sum(os.path.getsize(out / n) for n in names) <= 64 << 20
    arr = {n[:-4]: np.load(out / n) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arr.values())
    assert arr["loss"].shape == (1,) and float(arr["loss"][0]) == np.float32(d["final_loss"])
    assert arr["params_sample"].shape == arr["grads_sample"].shape and arr["params_sample"].size > 1 << 20
    assert np.abs(arr["grads_sample"]).max() > 0


def test_bench_spawns_its_ranks_through_the_launcher(dev):
    """`bench.py --gpus N` without a launcher around it runs `torch.distributed.run` as a child and forwards rank 0's line
    (tests/test_bench_launch_cpu.py holds the plumbing); here the real launcher on the one GPU of this box (`--spawn`: the
    N > 1 path at N = 1), with the gradient buckets really going through RCCL (forced collectives) — the line reports what
    the communicator saw, not the flag.  The reference's ranks: config/config.yaml:45-46, train.sh:6."""
    import json
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MRMT3_DDP_FORCE_COLLECTIVES"] = "1"
    r = subprocess.run([_sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--spawn", "--batch", "4", "--steps", "3",
                        "--warmup", "1", "--extra-batch", "0", "--no-inference", "--no-cpu-baseline", "--no-roofline"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["ranks_seen"] == 1 and d["launched_by"].startswith("bench.py --gpus 1 -> child")
    assert d["collectives"].startswith("rccl") and d["value"] > 0 and d["steps"] == 3
    # the multi-rank preflight ran: every stage left its line on stderr and its figures in the record
    for st in ("rccl_init", "bucket_allreduce", "stream_pick", "capture", "timed", "report"):
        assert "rank 0: stage %s" % st in r.stderr, (st, r.stderr[-1500:])
    pre = d["preflight"]
    assert len(pre["bucket_allreduce"]) == 5 and all(b["ms"] > 0 for b in pre["bucket_allreduce"])
    assert pre["capture"]["captured"] and pre["capture"]["graph_segments"] == 6 and pre["capture"]["replicas_identical"]
    assert pre["stream_pick"]["seconds"] < 1.5 and pre["rccl_init_seconds"] > 0
    # a rank that dies: its stage on stderr, ONE JSON line with "error" and "stage", exit code 1
    env_bad = dict(env, MRMT3_DDP_LAYERS_PER_BUCKET="not-a-number")
    r = subprocess.run([_sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--spawn", "--batch", "4", "--steps", "1",
                        "--warmup", "0", "--extra-batch", "0", "--no-inference", "--no-cpu-baseline", "--no-roofline"],
                       capture_output=True, text=True, env=env_bad, timeout=600)
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]
    e = json.loads(lines[0])
    assert e["value"] is None and e["stage"] == "model" and "ValueError" in e["error"], e
    assert "rank 0: FAILED at stage model" in r.stderr
    # more ranks than GPUs on this box: refused, nothing on stdout
    n = torch.cuda.device_count()
    r = subprocess.run([_sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n + 1)], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 2 and r.stdout == "" and "visible" in r.stderr
