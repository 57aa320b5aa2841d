"""The masked oracle itself, on the CPU: `oracle.t5_ref.forward_logits(..., drop=)` under the masks of
tests/_dropout_grads.DropPlan.  What tests/test_dropout_grads_gpu.py relies on is checked here: p = 0 is the oracle as it
was, the masked forward is a function autograd differentiates exactly, every one of the 24 dropout sites of the model moves
some gradient by far more than the GPU tests' bound when it is drawn from another stream, and the step salt reaches the masks.

small_cfg() (2 + 2 layers), B = 2, 64 mel frames, 32 target tokens, float64."""
import numpy as np
import pytest
import torch

from _dropout_grads import DropPlan, oracle_grads, oracle_loss, rel_l2, weights64
from optim_groups_ref import small_cfg

P = 0.1


@pytest.fixture(scope="module")
def case():
    from mrmt3.synthetic import synth_labels, synth_mel
    torch.set_num_threads(8)
    cfg = small_cfg()
    mel = torch.from_numpy(synth_mel(2, frames=64, seed=21))
    lab = torch.from_numpy(synth_labels(2, 32, full=False, seed=22, mean_len=20))
    assert (lab == -100).any() and (lab != -100).sum() >= 16
    return cfg, mel, lab


@pytest.fixture(scope="module")
def base(case):
    """The masked oracle's loss and gradients with every site on its own stream (shared, never modified)."""
    cfg, mel, lab = case
    plan = DropPlan(P, step=0)
    loss, _, grads = oracle_grads(cfg, mel, lab, drop=plan)
    return loss, grads, plan.names


def test_p0_plan_is_the_old_oracle_bit_for_bit(case):
    """`drop=` with p = 0 changes no bit of the logits, in fp32 (the dtype of the golden tests) and in float64, for a model
    with a memory encoder as well (the plan's memory sites are identity by construction)."""
    from mrmt3.synthetic import golden_weights
    from oracle import t5_ref
    cfg, mel, lab = case
    for variant, nseg in (("t5", 0), ("segmem_v2", 1), ("segmem_v1", 1), ("segmem_v2", 2)):
        sd32 = {k: torch.from_numpy(v) for k, v in golden_weights(cfg, nseg).items()}
        for sd, m in ((sd32, mel), ({k: v.double() for k, v in sd32.items()}, mel.double())):
            with torch.no_grad():
                kw = dict(variant=variant, segmem_length=16, segmem_num_layers=max(1, nseg))
                a = t5_ref.forward_logits(sd, cfg, m, lab, **kw)
                b = t5_ref.forward_logits(sd, cfg, m, lab, drop=DropPlan(0.0, step=3), **kw)
            assert torch.equal(a, b), (variant, nseg, a.dtype)


def test_site_walk_of_the_plan(base):
    """1 + 2 * 4 + 1 encoder sites, then 1 + 2 * 6 + 1 decoder sites, in the engine's order."""
    names = base[2]
    enc = ["encoder.emb"] + ["encoder." + n for n in ("att", "o", "g", "wo")] * 2 + ["encoder.out"]
    dec = ["decoder.emb"] + ["decoder." + n for n in ("att", "o", "catt", "co", "g", "wo")] * 2 + ["decoder.out"]
    assert names == enc + dec and len(names) == 24


def test_memory_encoder_consumes_ids_only_on_the_generic_path(case):
    """One memory layer (the engine's shortcut) draws no id; two draw 4 * 2 + 1 between the encoder's and the decoder's."""
    cfg, mel, lab = case
    for nseg, extra in ((1, 0), (2, 9)):
        plan = DropPlan(P, step=0)
        with torch.no_grad():
            oracle_loss(weights64(cfg, nseg, grad=False), cfg, mel, lab, "segmem_v2", segmem_num_layers=nseg, drop=plan)
        assert len(plan.names) == 24 + extra
        assert plan.names.index("decoder.emb") == 10 + extra
        assert [n for n in plan.names if n.startswith("segmem")] == (["segmem_encoder." + n for n in ("att", "o", "g", "wo")] * 2
                                                                     + ["segmem_encoder.out"])[:extra]


def test_masked_forward_is_what_autograd_differentiates(case, base):
    """The masks are constants, so the masked forward is smooth in the weights: central differences of the loss along three
    random directions (all weights at once, h = 1e-5 times the weights' norm scale) equal autograd's directional derivative
    to 1e-6 relative."""
    cfg, mel, lab = case
    _, grads, _ = base
    sd = weights64(cfg, grad=False)
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        v = {k: torch.randn(w.shape, generator=g, dtype=torch.float64) * w.std() for k, w in sd.items()}
        want = sum(float((grads[k] * v[k]).sum()) for k in sd)
        h = 1e-5
        with torch.no_grad():
            lp = oracle_loss({k: w + h * v[k] for k, w in sd.items()}, cfg, mel, lab, drop=DropPlan(P, step=0))[0].item()
            lm = oracle_loss({k: w - h * v[k] for k, w in sd.items()}, cfg, mel, lab, drop=DropPlan(P, step=0))[0].item()
        got = (lp - lm) / (2 * h)
        print("directional derivative: autograd %.12e central difference %.12e" % (want, got))
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)


def test_every_site_moves_a_gradient(case, base):
    """Each of the 24 sites in turn is drawn from an unused stream id (1000 + k); at least one gradient tensor must then
    move by rel-L2 >= 1e-2, 100 x the fp32 bound of the GPU tests, so those tests see a wrong id at any single site.  The
    table (site, most-moved tensor, rel-L2) is printed."""
    cfg, mel, lab = case
    _, grads, names = base
    sd = weights64(cfg)
    rows = []
    for k, name in enumerate(names):
        _, _, g = oracle_grads(cfg, mel, lab, drop=DropPlan(P, step=0, swap={k: 1000 + k}), sd=sd)
        moved = max((rel_l2(g[t], grads[t]), t) for t in grads if grads[t] is not None and grads[t].norm() > 0)
        rows.append((k + 1, name) + moved)
    print("\nsite  name            most-moved tensor                                             rel-L2")
    for sid, name, rel, t in rows:
        print("%4d  %-14s  %-60s  %.3e" % (sid, name, t, rel))
    print("minimum over the 24 sites: %.3e" % min(r[2] for r in rows))
    assert len(rows) == 24
    for sid, name, rel, t in rows:
        assert rel >= 1e-2, (sid, name, t, rel)


def test_step_salt_reaches_the_masks(case, base):
    """No counter, step 0 and step 1 are three different masked forwards."""
    cfg, mel, lab = case
    sd = weights64(cfg, grad=False)
    with torch.no_grad():
        losses = [oracle_loss(sd, cfg, mel, lab, drop=DropPlan(P, step=s))[0].item() for s in (None, 0, 1)]
    print("loss at step None / 0 / 1:", losses)
    assert losses[1] == base[0]
    assert len({round(l, 9) for l in losses}) == 3 and np.ptp(losses) > 1e-4
