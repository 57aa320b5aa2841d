"""Gradient accumulation in the trainer (`Trainer(accumulate_grad_batches=N)`, mrmt3/trainer.py) and in train.py, on the
MI355X: the accumulated gradient against the oracle's per-micro-batch autograd, the AdamW step against float64, N x B/N rows
against one step of B rows, graph replay against eager launches with dropout on (per-micro-batch salts), a partial cycle,
packed micro-batches, the bucket exchange (only in a cycle's last phase; two ranks against one process) and train.py's step
counting."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(variant, dtype, dev, **over):
    from mrmt3.synthetic import T5_SMALL
    cfg = dict(T5_SMALL, **over)
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        return T5ForConditionalGeneration(cfg, compute_dtype=dtype).load_golden().to(dev)
    from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
    return T5SegMemV2WithPrev(cfg, 1, 64, compute_dtype=dtype).load_golden().to(dev)


def _micro(dev, B=1, L=192, seed=0, full=False, mean_len=60):
    from mrmt3.synthetic import synth_mel, synth_labels
    mel = torch.from_numpy(synth_mel(B, seed=seed + 1)).to(dev)
    lab = torch.from_numpy(synth_labels(B, L, full=full, seed=seed + 2, mean_len=mean_len)).to(dev)
    return mel, lab


def _rel(a, b):
    return float((a - b).norm() / b.norm()) if b.norm() > 0 else float(a.norm())


def _adamw64(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8, wd=0.01):
    """torch.optim.AdamW's single-tensor update in float64 (numpy arrays); returns (p, m, v)."""
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v


def _f64(t):
    return t.detach().double().cpu().numpy()


def test_accumulated_gradient_equals_oracle_mean_and_adamw_in_float64(dev):
    """fp32 engine, p = 0, N = 2, padded labels with different token counts per micro-batch: G / 2 is the mean of the
    oracle's per-micro-batch float64 autograd gradients (each micro-batch's CE a mean over its own tokens), and the
    parameters are one float64 AdamW step on that gradient at the scheduled learning rate."""
    from mrmt3.synthetic import T5_SMALL, golden_weights
    from mrmt3.trainer import Trainer
    from oracle import t5_ref
    micro = [_micro(dev, B=2, L=256, seed=10, mean_len=50), _micro(dev, B=2, L=256, seed=20, mean_len=150)]
    counts = [int((lab != -100).sum()) for _, lab in micro]
    assert counts[0] != counts[1], counts
    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    p0 = _f64(m.flat.P)
    tr = Trainer(m, lr=1e-3, lr_lambda=lambda s: 0.5 + 0.25 * s, graph=False, accumulate_grad_batches=2)
    losses = [float(tr.train_step(mel, lab).item()) for mel, lab in micro]
    torch.cuda.synchronize()
    assert tr.optimizer_steps == 1 and tr.pending_micro_batches == 0 and int(tr.step_dev.item()) == 1
    torch.set_num_threads(8)
    want = {}
    for (mel, lab), got_loss in zip(micro, losses):
        sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in golden_weights(T5_SMALL, 0).items()}
        logits = t5_ref.forward_logits(sd, T5_SMALL, mel.cpu().double(), lab.cpu())
        loss = t5_ref.ce_loss(logits, lab.cpu())
        loss.backward()
        assert abs(float(loss.item()) - got_loss) < 2e-5, (float(loss.item()), got_loss)    # the undivided micro loss
        for k, v in sd.items():
            if v.grad is not None:
                want[k] = want.get(k, 0) + v.grad / 2
    worst = 0.0
    for k in m.flat.shapes:
        g = m.flat.grad(k).detach().double().cpu() / 2
        if k not in want or want[k].norm() == 0:
            assert g.norm() < 1e-7, k
            continue
        r = _rel(g, want[k])
        worst = max(worst, r)
        assert r <= 5e-6, (k, r)
    print("worst rel-L2 against the float64 oracle: %.2e" % worst)
    p64, _, _ = _adamw64(p0, _f64(m.flat.G) / 2, 0.0, 0.0, lr=1e-3 * 0.5, step=1)
    assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6


@pytest.mark.parametrize("variant", ["t5", "segmem_v2_with_prev"])
def test_two_half_micro_batches_equal_one_full_batch(dev, variant):
    """fp32, p = 0, full-length labels (equal token counts: the mean of the micro-batch means is the batch mean): N = 2 with
    B/2 rows each equals N = 1 with B rows, gradient and parameters within rel-L2 2e-6."""
    from mrmt3.synthetic import synth_labels
    from mrmt3.trainer import Trainer
    mel, lab = _micro(dev, B=2, L=192, seed=30, full=True)
    prev = torch.from_numpy(synth_labels(2, 192, full=False, seed=33, mean_len=80)).to(dev) \
        if variant != "t5" else None
    runs = {}
    for n in (1, 2):
        m = _model(variant, torch.float32, dev, dropout_rate=0.0)
        tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=n)
        rows = [slice(0, 2)] if n == 1 else [slice(0, 1), slice(1, 2)]
        for r in rows:
            tr.train_step(mel[r], lab[r], None if prev is None else prev[r].clone())
        torch.cuda.synchronize()
        assert tr.optimizer_steps == 1
        runs[n] = ({k: m.flat.grad(k).detach().cpu().clone() / n for k in m.flat.shapes}, m.flat.P.detach().cpu().clone())
    for k, g in runs[1][0].items():
        if g.norm() == 0:
            assert runs[2][0][k].norm() < 1e-7, k
            continue
        assert _rel(runs[2][0][k], g) <= 2e-6, (k, _rel(runs[2][0][k], g))
    assert _rel(runs[2][1], runs[1][1]) <= 2e-6


@pytest.mark.parametrize("packed", [False, True])
def test_replayed_accumulation_equals_eager_bitwise_with_dropout(dev, packed):
    """bf16, dropout 0.1, N = 2 (the first and last phases are each captured after their two eager warm-up uses, then
    replayed): the graph trainer equals the eager trainer in every micro-batch loss and in the final weights and moments, bit
    for bit.  Dense: both micro-batches of a cycle are the SAME batch on the same weights (the optimizer steps after the
    second), so their losses differ only through the dropout masks: the two micro-batches drew different salts.  Packed: the
    two micro-batches of a cycle take different capacities (signatures of capacity and phase)."""
    from mrmt3.trainer import Trainer
    a = _micro(dev, B=3, L=192, seed=40, mean_len=40)
    b = (a[0], a[1].clone())
    b[1][:, :150] = 5                              # 150-token rows: another packed capacity than a's
    b[1][:, 150:] = -100
    order = [a, b] * 4 if packed else [a, a] * 3
    runs = {}
    for use_graph in (False, True):
        m = _model("t5", torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=use_graph, pack_targets=packed, accumulate_grad_batches=2)
        assert tr.salt_dev is not tr.step_dev
        if packed:
            assert len({tr.pack_capacity(x[1]) for x in (a, b)} - {None}) == 2
        losses = [float(tr.train_step(*x).item()) for x in order]
        torch.cuda.synchronize()
        n = len(order)
        assert tr.optimizer_steps == n // 2 and int(tr.step_dev.item()) == n // 2 and int(tr.salt_dev.item()) == n
        assert tr.graph_captured == use_graph
        if use_graph:
            assert sorted(s[-1] for s in tr._graphs) == ["first", "last"], list(tr._graphs)
            assert all(len(s) == (7 if packed else 6) for s in tr._graphs), list(tr._graphs)
        runs[use_graph] = (losses, m.flat.P.clone(), m.flat.M.clone(), m.flat.V.clone())
        tr.close()
    le, lg = runs[False][0], runs[True][0]
    assert np.allclose(le, lg, rtol=0, atol=2e-6), list(zip(le, lg))
    for x, y in zip(runs[False][1:], runs[True][1:]):
        assert torch.equal(x, y)
    if not packed:
        assert min(abs(le[i] - le[i + 1]) for i in range(0, len(le), 2)) > 1e-4, le    # same batch and weights, other masks
    # N = 1 keeps the optimizer step counter as the salt: the masks of the plain step
    tr = Trainer(_model("t5", torch.bfloat16, dev), lr=1e-3, graph=False)
    assert tr.salt_dev is tr.step_dev and tr.engine.step_dev is tr.step_dev


def test_partial_cycle_applies_the_sum_over_n_and_counts_one_step(dev, tmp_path):
    """N = 4, three micro-batches, then finish_accumulation(): the parameters move only then, by one float64 AdamW step on
    G / 4; the LR lambda and the AdamW step counter advance once per optimizer step; a checkpoint is refused while
    micro-batches are pending."""
    from mrmt3.trainer import Trainer
    seen = []

    def lam(s):
        seen.append(s)
        return 0.5 + 0.25 * s

    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    p0 = _f64(m.flat.P)
    tr = Trainer(m, lr=1e-3, lr_lambda=lam, graph=False, accumulate_grad_batches=4)
    assert not tr.finish_accumulation()             # nothing pending: nothing happens
    for s in range(3):
        tr.train_step(*_micro(dev, seed=50 + 10 * s))
    torch.cuda.synchronize()
    assert tr.pending_micro_batches == 3 and tr.optimizer_steps == 0 and int(tr.step_dev.item()) == 0
    assert np.array_equal(_f64(m.flat.P), p0)       # no optimizer step yet
    with pytest.raises(RuntimeError, match="finish_accumulation"):
        tr.save_checkpoint(str(tmp_path / "x.ckpt"))
    g = _f64(m.flat.G)
    assert tr.finish_accumulation()
    torch.cuda.synchronize()
    assert tr.pending_micro_batches == 0 and tr.optimizer_steps == 1 and int(tr.step_dev.item()) == 1
    assert not tr.finish_accumulation()
    p64, _, _ = _adamw64(p0, g / 4, 0.0, 0.0, lr=1e-3 * 0.5, step=1)
    assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6
    assert set(seen) == {0}
    p1, m1, v1 = _f64(m.flat.P), _f64(m.flat.M), _f64(m.flat.V)
    # a full cycle afterwards: lr lambda(1), AdamW step 2
    for s in range(4):
        tr.train_step(*_micro(dev, seed=90 + 10 * s))
        assert tr.optimizer_steps == (1 if s < 3 else 2)
    torch.cuda.synchronize()
    assert set(seen) == {0, 1} and abs(float(tr.lr_dev.item()) - 1e-3 * 0.75) < 1e-9
    assert int(tr.step_dev.item()) == 2
    p64, _, _ = _adamw64(p1, _f64(m.flat.G) / 4, m1, v1, lr=1e-3 * 0.75, step=2)
    assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6
    tr.save_checkpoint(str(tmp_path / "y.ckpt"))
    blob = torch.load(tmp_path / "y.ckpt", weights_only=False)
    assert blob["global_step"] == 2 and blob["mrmt3"]["dropout_salt"] == 7


def test_packed_micro_batches_equal_dense_accumulation(dev):
    """pack_targets with N = 2 and a different Tcap per micro-batch equals the dense accumulation: fp32 engine, p = 0,
    every gradient tensor within rel-L2 2e-6."""
    from mrmt3.trainer import Trainer
    micro = [_micro(dev, B=3, L=192, seed=60, mean_len=40), _micro(dev, B=3, L=192, seed=70, full=True)]
    micro[1][1][:, 100:] = -100                    # 300 tokens: Tcap 512 (the first micro-batch: 256)
    G = {}
    for packed in (False, True):
        m = _model("t5", torch.float32, dev, dropout_rate=0.0)
        tr = Trainer(m, lr=1e-3, graph=False, pack_targets=packed, accumulate_grad_batches=2)
        if packed:
            caps = [tr.pack_capacity(lab) for _, lab in micro]
            assert None not in caps and caps[0] != caps[1], caps
        for mel, lab in micro:
            tr.train_step(mel, lab)
        torch.cuda.synchronize()
        G[packed] = {k: m.flat.grad(k).detach().cpu().clone() for k in m.flat.shapes}
    for k, g in G[False].items():
        if g.norm() == 0:
            assert G[True][k].norm() < 1e-7, k
            continue
        assert _rel(G[True][k], g) <= 2e-6, (k, _rel(G[True][k], g))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _recording_fires(tr):
    """Record (micro-batch index in its cycle, bucket) of every bucket sent (a second fire of a bucket in a step is a no-op)."""
    fires, orig = [], tr.buckets._fire

    def rec(idx):
        if idx not in tr.buckets._fired:
            fires.append((tr.pending_micro_batches, idx))
        return orig(idx)
    tr.buckets._fire = rec
    return fires


def test_forced_collectives_fire_only_in_the_last_phase(dev, monkeypatch):
    """One rank with the collectives forced: the buckets are exchanged only in a cycle's last micro-batch, in eager and
    replayed steps (three cycles of N = 2: both phases captured), and the result is that of the trainer without them."""
    from mrmt3.trainer import Trainer
    port = _free_port()
    data = [_micro(dev, B=2, L=128, seed=100 + 10 * i) for i in range(2)]
    P = {}
    monkeypatch.setenv("MRMT3_DDP_FORCE_COLLECTIVES", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        for use_graph in (False, True):
            m = _model("t5", torch.bfloat16, dev, dropout_rate=0.0)
            tr = Trainer(m, lr=1e-3, graph=use_graph, accumulate_grad_batches=2)
            assert tr.buckets.active
            fires = _recording_fires(tr)
            for i in range(6):
                tr.train_step(*data[i % 2])
            torch.cuda.synchronize()
            assert tr.graph_captured == use_graph and tr.optimizer_steps == 3
            nb = len(tr.buckets.buckets)
            assert len(fires) == 3 * nb and all(i == 1 for i, _ in fires), fires
            if use_graph:
                last = [c for s, c in tr._graphs.items() if s[-1] == "last"][0]
                first = [c for s, c in tr._graphs.items() if s[-1] == "first"][0]
                assert len(last.segments) == nb and first.segments == []
            P[use_graph] = m.flat.P.clone()
            tr.close()
            p0 = _model("t5", torch.bfloat16, dev, dropout_rate=0.0).flat.P.clone()
    finally:
        dist.destroy_process_group()
    monkeypatch.delenv("MRMT3_DDP_FORCE_COLLECTIVES")
    m = _model("t5", torch.bfloat16, dev, dropout_rate=0.0)
    tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=2)
    assert not tr.buckets.active
    for i in range(6):
        tr.train_step(*data[i % 2])
    torch.cuda.synchronize()
    assert torch.equal(P[False], P[True])
    assert _rel(P[False] - p0, m.flat.P - p0) < 1e-3


def _rank_worker(rank, world, port, q, micro):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "mr-mt3_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mrmt3.trainer import Trainer
        m = _model("t5", torch.bfloat16, dev, dropout_rate=0.0)
        tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=len(micro))
        fires = _recording_fires(tr)
        losses = [float(tr.train_step(mel.to(dev), lab.to(dev)).item()) for mel, lab in micro]
        torch.cuda.synchronize()
        q.put((rank, m.flat.G.cpu().numpy(), m.flat.P.cpu().numpy(), losses, fires, len(tr.buckets.buckets),
               tr.optimizer_steps))
    finally:
        dist.destroy_process_group()


def test_two_ranks_accumulating_equal_one_process_on_the_global_micro_batches(dev):
    """Two ranks on one GPU, N = 2 each, exchange only in the second micro-batch: the exchanged gradient is the sum over the
    four micro-batches that ONE process accumulating all four (N = 4) holds (same per-micro-batch gradients, another order of
    the f32 additions), both ranks hold identical replicas, and their step equals that process's."""
    from mrmt3.synthetic import synth_mel, synth_labels
    micro = [(torch.from_numpy(synth_mel(2, seed=200 + i)), torch.from_numpy(synth_labels(2, 128, seed=300 + i)))
             for i in range(4)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, micro[2 * r:2 * r + 2])) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, g0, p0, l0, f0, nb, s0), (_, g1, p1, l1, f1, _, s1) = res
    assert s0 == s1 == 1
    assert np.array_equal(g0, g1) and np.array_equal(p0, p1)
    for f in (f0, f1):
        assert len(f) == nb and all(i == 1 for i, _ in f), f
    from mrmt3.trainer import Trainer
    m = _model("t5", torch.bfloat16, dev, dropout_rate=0.0)
    start = m.flat.P.detach().cpu().numpy().copy()
    tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=4)
    losses = [float(tr.train_step(mel.to(dev), lab.to(dev)).item()) for mel, lab in micro]
    torch.cuda.synchronize()
    g = m.flat.G.cpu().numpy()
    assert np.linalg.norm(g0 - g) / np.linalg.norm(g) < 1e-5
    for r, lr_ in ((0, l0), (1, l1)):                     # each rank logs the rank mean of its micro-batch losses
        assert np.allclose(lr_, [(losses[i] + losses[2 + i]) / 2 for i in range(2)], rtol=0, atol=2e-6), (lr_, losses)
    du, dw = p0 - start, m.flat.P.cpu().numpy() - start
    assert np.linalg.norm(du - dw) / np.linalg.norm(dw) < 1e-3


def test_train_py_counts_optimizer_steps(dev, tmp_path, monkeypatch, capsys):
    """train.py, synthetic=true grad_accum=2 max_steps=3: 6 micro-batches, 3 optimizer steps, 3 schedule steps, a step line
    per optimizer step, and the checkpoint holds step 3."""
    import train
    import utils
    from mrmt3 import trainer as trainer_mod
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
grad_accum: 1
optim:
  lr: 2e-4
  warmup_steps: 10
  num_epochs: ${num_epochs}
  num_steps_per_epoch: 100
  min_lr: 1e-4
trainer:
  log_every_n_steps: 1
  accumulate_grad_batches: ${grad_accum}
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
    sched, micro, made = [], [], []
    orig_lam, orig_step, orig_init = utils.cosine_warmup_lambda, trainer_mod.Trainer.train_step, trainer_mod.Trainer.__init__

    def lam_factory(*a, **k):
        f = orig_lam(*a, **k)

        def g(s):
            sched.append(s)
            return f(s)
        return g

    def step(self, *a, **k):
        micro.append(self.optimizer_steps)
        return orig_step(self, *a, **k)

    def init(self, *a, **k):
        made.append(self)
        orig_init(self, *a, **k)

    monkeypatch.setattr(utils, "cosine_warmup_lambda", lam_factory)
    monkeypatch.setattr(trainer_mod.Trainer, "train_step", step)
    monkeypatch.setattr(trainer_mod.Trainer, "__init__", init)
    out = tmp_path / "out"
    train.main(["--config-dir", str(tmp_path / "cfg"), "--config-name", "config", "+synthetic=True", "grad_accum=2",
                "+max_steps=3", f"+output_dir={out}"])
    tr, = made
    assert tr.accumulate == 2
    assert micro == [0, 0, 1, 1, 2, 2]                    # 6 micro-batches over 3 optimizer steps
    assert tr.optimizer_steps == 3 and int(tr.step_dev.item()) == 3 and int(tr.salt_dev.item()) == 6
    assert sorted(set(sched)) == [0, 1, 2, 3]             # the lr of steps 0, 1, 2, and the checkpoint's next lr
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("step ")]
    assert [x.split()[1] for x in lines] == ["0", "1", "2"], lines
    blob = torch.load(out / "MT3Net_Slakh" / "version_0" / "checkpoints" / "last.ckpt", weights_only=False)
    assert blob["global_step"] == 3 and blob["lr_schedulers"][0]["last_epoch"] == 3
    assert blob["mrmt3"]["dropout_salt"] == 6
