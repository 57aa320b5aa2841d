"""Gradient accumulation, host side (no GPU): the option read from a composed config the way the reference's configs spell
it (`grad_accum` + `trainer.accumulate_grad_batches: ${grad_accum}`), the resume arithmetic and the batch iterator counting
OPTIMIZER steps, and the trainer's refusal of a count below one."""
import sys

import pytest
import torch

TOP = """
seed: 365
grad_accum: 1
trainer:
  precision: 32
  accumulate_grad_batches: ${grad_accum}
  log_every_n_steps: 50
"""


@pytest.fixture()
def cfgdir(tmp_path):
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "bare.yaml").write_text("seed: 365\ntrainer:\n  precision: 32\n")
    (tmp_path / "toplevel.yaml").write_text("seed: 365\ngrad_accum: 3\ntrainer:\n  precision: 32\n")
    return str(tmp_path)


def test_accumulation_is_read_from_the_composed_config(cfgdir):
    import train
    from mrmt3 import hydra_lite
    assert train.accumulate_grad_batches(hydra_lite.compose(cfgdir, "config", [])) == 1
    assert train.accumulate_grad_batches(hydra_lite.compose(cfgdir, "config", ["grad_accum=4"])) == 4
    assert train.accumulate_grad_batches(hydra_lite.compose(cfgdir, "config", ["trainer.accumulate_grad_batches=2"])) == 2
    assert train.accumulate_grad_batches(hydra_lite.compose(cfgdir, "toplevel", [])) == 3     # falls back to grad_accum
    assert train.accumulate_grad_batches(hydra_lite.compose(cfgdir, "bare", [])) == 1         # neither key: 1


@pytest.mark.parametrize("n", [0, -1, 1.5])
def test_trainer_refuses_a_count_below_one_or_fractional(n):
    from mrmt3.trainer import Trainer
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(None, accumulate_grad_batches=n)             # refused before the model is looked at


def _loader(tmp_path, n_train):
    from mrmt3 import hydra_lite
    (tmp_path / "toyset_acc.py").write_text(
        "import torch\n"
        "from torch.utils.data import Dataset\n"
        "class Toy(Dataset):\n"
        "    def __init__(self, n): self.n = n\n"
        "    def __len__(self): return self.n\n"
        "    def __getitem__(self, i): return torch.full((1, 4), float(i)), torch.full((1, 2), i, dtype=torch.int64)\n"
        "def collate(batch):\n"
        "    return torch.cat([b[0] for b in batch]), torch.cat([b[1] for b in batch])\n")
    if str(tmp_path) not in sys.path:
        sys.path.insert(0, str(tmp_path))
    cfg = hydra_lite._wrap({
        "seed": 365,
        "dataset": {"train": {"_target_": "toyset_acc.Toy", "n": n_train}, "val": {"_target_": "toyset_acc.Toy", "n": 2},
                    "collate_fn": "toyset_acc.collate"},
        "dataloader": {"train": {"batch_size": 1, "shuffle": True}, "val": {"batch_size": 1, "shuffle": False}}})
    import train
    return train.real_loaders(cfg)[0]


def test_resume_position_counts_optimizer_steps():
    """5 batches per epoch, N = 2: steps end after batches 2, 4 and 5 (the partial cycle at the epoch's end) — 3 steps per
    epoch.  N = 1 keeps the plain arithmetic."""
    import train
    assert [train.resume_position(s, 5, 2) for s in range(8)] == \
        [(0, 0), (0, 2), (0, 4), (1, 0), (1, 2), (1, 4), (2, 0), (2, 2)]
    assert [train.resume_position(s, 5, 5) for s in range(3)] == [(0, 0), (1, 0), (2, 0)]
    assert [train.resume_position(s, 5, 8) for s in range(3)] == [(0, 0), (1, 0), (2, 0)]   # N > len: one step per epoch
    assert [train.resume_position(s, 5) for s in range(7)] == [(s // 5, s % 5) for s in range(7)]


@pytest.mark.parametrize("n_acc", [2, 3])
def test_loader_batches_count_optimizer_steps_and_resume_at_a_cycle_boundary(tmp_path, n_acc):
    """max_steps caps optimizer steps; a run resumed from any optimizer step continues with exactly the batches the
    interrupted run had not consumed, whole cycles included."""
    import train
    tl = _loader(tmp_path, n_train=5)                        # 5 batches per epoch
    dev = torch.device("cpu")
    epochs = 2
    per_epoch = -(-5 // n_acc)
    full = [(ep, int(x[0, 0])) for ep, x, _, _ in train.loader_batches(tl, dev, epochs, None, accumulate=n_acc)]
    assert [e for e, _ in full] == [0] * 5 + [1] * 5
    # max_steps = per_epoch + 1: the whole first epoch, then one cycle of the second
    capped = list(train.loader_batches(tl, dev, epochs, per_epoch + 1, accumulate=n_acc))
    assert [b[0] for b in capped] == [0] * 5 + [1] * n_acc
    for done in range(per_epoch * epochs + 1):
        ep0, skip = train.resume_position(done, len(tl), n_acc)
        rest = [(ep, int(x[0, 0])) for ep, x, _, _ in
                train.loader_batches(tl, dev, epochs, None, ep0, done, skip=skip, accumulate=n_acc)]
        consumed = min(5, (done % per_epoch) * n_acc) + 5 * (done // per_epoch)
        assert rest == full[consumed:], (done, rest)
        capped = list(train.loader_batches(tl, dev, epochs, done + 1, ep0, done, skip=skip, accumulate=n_acc))
        if done < per_epoch * epochs:                        # exactly one more optimizer step's batches
            pos = consumed % 5
            assert len(capped) == min(n_acc, 5 - pos), (done, len(capped))
