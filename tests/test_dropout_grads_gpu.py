"""The training step WITH dropout on the MI355X against autograd: the engine's loss, logits and every gradient tensor
(`training=True`, p = 0.1) against the float64 oracle run under exactly the masks the kernels draw
(tests/_dropout_grads.DropPlan; tests/test_dropout_grads_cpu.py shows that a wrong stream id at any single site moves some
gradient by rel-L2 >= 1e-1).  Legs: A the fp32 engine, every variant and three values of the step counter; B packed decoder
rows; C the bf16 engine at the shape where the fused projection + row kernels, the one-pass attention backward and the
grouped weight-gradient launch carry the dropout; D what the trainer's `step_dev` / `salt_dev` feed the kernels.

All at small_cfg(dropout_rate=0.1) (2 + 2 layers) with the golden weights."""
import numpy as np
import pytest
import torch

from _dropout_grads import DropPlan, oracle_grads, oracle_loss, rel_l2, weights64
from optim_groups_ref import small_cfg

pytestmark = pytest.mark.gpu
P = 0.1
V = 1536


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(8)
    return torch.device("cuda:0")


def _cfg():
    return small_cfg(dropout_rate=P)


def _model(variant, dtype, dev, nseg=1):
    import importlib
    mod, cls = {"t5": ("models.t5", "T5ForConditionalGeneration"), "segmem_v1": ("models.t5_segmem", "T5SegMem"),
                "segmem_v2": ("models.t5_segmem_v2", "T5SegMemV2"),
                "segmem_v2_with_prev": ("models.t5_segmem_v2_with_prev", "T5SegMemV2WithPrev")}[variant]
    M = getattr(importlib.import_module(mod), cls)
    m = M(_cfg(), compute_dtype=dtype) if variant == "t5" else M(_cfg(), nseg, 64, compute_dtype=dtype)
    return m.load_golden().to(dev)


def _inputs(B, frames, L, seed, mean_len):
    from mrmt3.synthetic import synth_labels, synth_mel
    mel = torch.from_numpy(synth_mel(B, frames=frames, seed=seed))
    lab = torch.from_numpy(synth_labels(B, L, full=False, seed=seed + 1, mean_len=mean_len))
    prev = torch.from_numpy(synth_labels(B, L, full=False, seed=seed + 2, mean_len=mean_len))
    assert (lab == -100).any() and (prev == -100).any()
    return mel, lab, prev


def _engine_step(m, mel, lab, prev, step, pack=None):
    """One forward + backward of the engine with training=True, driven like Trainer._step_body: (loss, logits or None,
    {name: grad}).  step: the value of the device step counter (None: no counter attached)."""
    from mrmt3 import lib
    eng, dev = m.engine, mel.device
    m.flat.ensure_grads()
    eng.begin_step()
    eng.step_dev = None if step is None else torch.tensor([step], device=dev, dtype=torch.int32)
    targets = lab.reshape(-1) if pack is None else pack.targets
    prev = None if prev is None else prev.clone()
    kw = dict(training=True, need_grad=True, pack=pack)
    if eng.dt == torch.bfloat16:
        logits = None
        dec, tape = eng.forward(mel, lab, prev, want_logits=False, **kw)
        loss, dl = lib.lmhead_cross_entropy(dec, eng.W("lm_head"), targets, want_grad=True, grad_dtype=torch.bfloat16)
    else:
        logits, tape = eng.forward(mel, lab, prev, **kw)
        loss, dl = lib.cross_entropy(logits.reshape(-1, V), targets, want_grad=True, grad_dtype=torch.float32)
    m.flat.G.zero_()
    eng.backward(tape, dl)
    torch.cuda.synchronize()
    eng.step_dev = None
    grads = {k: m.flat.grad(k).detach().float().cpu().clone() for k in m.flat.shapes}
    return float(loss.item()), None if logits is None else logits.detach().cpu(), grads


def _check_fp32(tag, loss, grads, ref_loss, ref_grads):
    """The bounds of test_fp32_gradients_match_oracle: |loss - oracle| < 2e-5, every gradient tensor rel-L2 < 1e-4, a tensor
    whose oracle gradient is zero has norm < 1e-7."""
    worst = (0.0, "")
    bad = []
    for k, g in grads.items():
        r = ref_grads.get(k)
        if r is None or r.norm() == 0:
            if g.norm() >= 1e-7:
                bad.append((k, "oracle 0", float(g.norm())))
            continue
        rel = rel_l2(g, r)
        worst = max(worst, (rel, k))
        if not rel < 1e-4:
            bad.append((k, rel))
    print("%s: |d loss| %.2e, worst gradient rel-L2 %.3e (%s)" % (tag, abs(loss - ref_loss), worst[0], worst[1]))
    assert abs(loss - ref_loss) < 2e-5, (tag, loss, ref_loss)
    assert not bad, (tag, bad)


# ---- A: the fp32 engine against the masked oracle ------------------------------------------------------------------------
A_CASES = [("t5", 0), ("segmem_v2_with_prev", 1), ("segmem_v1", 1), ("segmem_v2", 2)]


@pytest.fixture(scope="module")
def a_inputs():
    return _inputs(2, 256, 64, seed=31, mean_len=40)


@pytest.mark.parametrize("step", [None, 0, 1000003])
@pytest.mark.parametrize("variant,nseg", A_CASES, ids=["%s-%d" % c for c in A_CASES])
def test_fp32_engine_matches_the_masked_oracle(dev, a_inputs, variant, nseg, step):
    """B = 2, 256 frames, 64 target tokens with -100 padding.  One memory layer is the engine's shortcut (no site id drawn),
    two the generic stack whose p = 0 sites still consume ids.  Loss and gradients to the fp32 bounds (see _check_fp32); the
    logits of the same training forward per element to 2e-4, the atol of test_fp32_logits_match_reference."""
    mel, lab, prev = a_inputs
    prev = prev if variant == "segmem_v2_with_prev" else None
    m = _model(variant, torch.float32, dev, nseg)
    loss, logits, grads = _engine_step(m, mel.to(dev), lab.to(dev), None if prev is None else prev.to(dev), step)
    ref_loss, ref_logits, ref_grads = oracle_grads(_cfg(), mel, lab, variant, prev, nseg, drop=DropPlan(P, step=step))
    dmax = float((logits.double() - ref_logits).abs().max())
    print("%s step %s: logits max|d| %.3e" % (variant, step, dmax))
    assert dmax < 2e-4, dmax
    _check_fp32("%s/%d step %s" % (variant, nseg, step), loss, grads, ref_loss, ref_grads)


# ---- B: packed decoder rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [None, 7])
def test_packed_fp32_engine_matches_the_masked_oracle(dev, step):
    """t5, B = 2, 256-token rows of 150 and 37 scored tokens: T = 187 rows packed into Tcap = 256, the second row starting
    off a 64-row tile.  The decoder's row-wise masks are keyed by the packed row, its attention masks by the row's own
    (b, h, q, k).  Same bounds as the dense leg; the logits are compared on the T packed rows."""
    from mrmt3 import lib, packing
    cfg = _cfg()
    mel, lab, _ = _inputs(2, 256, 256, seed=41, mean_len=100)
    lengths = [150, 37]
    rs = np.random.RandomState(3)
    lab = torch.from_numpy(rs.randint(3, 1391, size=(2, 256)).astype(np.int64))
    for b, n in enumerate(lengths):
        lab[b, n - 1] = 1
        lab[b, n:] = -100
    assert packing.row_lengths(lab.numpy()).tolist() == lengths
    tcap = packing.capacity(lengths, 2, 256)
    assert tcap == 256 > sum(lengths)
    pl = lib.pack_plan(lab.to(dev).contiguous(), tcap, cfg["decoder_start_token_id"], cfg["pad_token_id"])
    m = _model("t5", torch.float32, dev)
    loss, logits, grads = _engine_step(m, mel.to(dev), lab.to(dev), None, step, pack=pl)
    assert int(pl.err.item()) == 0
    ref_loss, ref_logits, ref_grads = oracle_grads(cfg, mel, lab, drop=DropPlan(P, step=step, pack_lengths=lengths, tcap=tcap))
    want = torch.cat([ref_logits[b, :n] for b, n in enumerate(lengths)])
    dmax = float((logits[:sum(lengths)].double() - want).abs().max())
    print("packed step %s: logits max|d| %.3e" % (step, dmax))
    assert dmax < 2e-4, dmax
    _check_fp32("packed step %s" % step, loss, grads, ref_loss, ref_grads)


# ---- C: the bf16 engine where the fused kernels carry the dropout ----------------------------------------------------------
_C_REF = {}


def _c_reference(variant):
    if variant not in _C_REF:
        mel, lab, prev = _inputs(4, 256, 256, seed=51, mean_len=150)
        prev = prev if variant == "segmem_v2_with_prev" else None
        ref = oracle_grads(_cfg(), mel, lab, variant, prev, drop=DropPlan(P, step=5))
        _C_REF[variant] = (mel, lab, prev, ref[0], ref[2])
    return _C_REF[variant]


@pytest.mark.parametrize("fuse_rows", [None, 7])
@pytest.mark.parametrize("variant", ["t5", "segmem_v2_with_prev"])
def test_bf16_engine_fused_dropout_paths_match_the_masked_oracle(dev, knobs, variant, fuse_rows):
    """B = 4, 256 frames, 256 tokens: 1024 encoder and 1024 decoder rows.  Default `fuse_rows` (norm backward and gated-GELU
    backward fused into the data-gradient products) and 7 (also the forward projection + add + norm with `out_drop`); the
    one-pass attention backward from one (batch, head) pair up and the fused wi + GEGLU launch from 1024 rows (two dispatch
    thresholds lowered to this shape; the kernels are the ones the benchmark's step runs).  The dispatch counters must show that the fused wi + GEGLU,
    both (or all three) fused row kernels, the one-pass backward and the grouped weight-gradient launch ran in this step —
    every site of it has p = 0.1 but the memory encoder's.  Bounds: the project's bf16 gradient rule against autograd
    (test_bf16_gradients_vs_oracle_autograd): loss within 2e-3, every tensor cosine > 0.9995 and rel-L2 < 3e-2."""
    from mrmt3 import lib
    knobs.set("MRMT3_ATTN_ONEPASS_MIN_BH", 1)
    knobs.set("MRMT3_GEGLU_FUSED_MIN_ROWS", 1024)        # (the fused wi + GEGLU launch is taken from 2048 rows by default)
    mel, lab, prev, ref_loss, ref_grads = _c_reference(variant)
    m = _model(variant, torch.bfloat16, dev)
    if fuse_rows is not None:
        m.engine.fuse_rows = fuse_rows
    lib.dispatch_counts(reset=True)
    loss, _, grads = _engine_step(m, mel.to(dev), lab.to(dev), None if prev is None else prev.to(dev), 5)
    c = lib.dispatch_counts()
    ran = ["gemm_nt_geglu", "gemm_nt_normbwd", "gemm_nt_geglubwd", "attn_bwd_onepass", "tn_group"]
    if (m.engine.fuse_rows & 1):
        ran.append("gemm_nt_addnorm")
    print({k: c[k] for k in ran})
    assert m.engine.fuse_rows & 6 == 6
    for k in ran:
        assert c[k] > 0, (k, c)
    assert c["gemm_nt_geglu"] >= 4 and c["gemm_nt_geglubwd"] >= 4 and c["attn_bwd_onepass"] >= 4, c
    bad, worst = [], (0.0, "")
    for k, g in grads.items():
        r = ref_grads.get(k)
        if r is None or r.norm() == 0:
            if g.norm() >= 1e-6:
                bad.append((k, "oracle 0", float(g.norm())))
            continue
        cos = torch.nn.functional.cosine_similarity(g.double().flatten(), r.flatten(), dim=0).item()
        rel = rel_l2(g, r)
        worst = max(worst, (rel, k))
        print("  %-62s rel-L2 %.3e cos %.6f" % (k, rel, cos))
        if not (cos > 0.9995 and rel < 3e-2):
            bad.append((k, cos, rel))
    print("%s fuse_rows %d: |d loss| %.2e, worst rel-L2 %.3e (%s)" % (variant, m.engine.fuse_rows, abs(loss - ref_loss), *worst))
    assert abs(loss - ref_loss) < 2e-3, (loss, ref_loss)
    assert not bad, bad


# ---- D: the trainer's salt -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def d_inputs():
    return _inputs(2, 256, 64, seed=61, mean_len=40)


@pytest.fixture(scope="module")
def adamw_trajectory(d_inputs):
    """Four AdamW steps (torch.optim.AdamW, lr 1e-3, its defaults = the trainer's) on the float64 oracle, step n under the
    masks of step counter n: the loss of every step."""
    torch.set_num_threads(8)
    mel, lab, _ = d_inputs
    cfg = _cfg()
    sd = weights64(cfg)
    opt = torch.optim.AdamW(list(sd.values()), lr=1e-3)
    losses = []
    for n in range(4):
        opt.zero_grad()
        loss, _ = oracle_loss(sd, cfg, mel, lab, drop=DropPlan(P, step=n))
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    return losses


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_steps_draw_the_masks_of_their_step_counter(dev, d_inputs, adamw_trajectory, graph):
    """fp32 trainer, lr 1e-3: the loss of step n is the masked oracle's with step = n at the weights n reference AdamW steps
    have reached, within 5e-5 (the atol of test_fp32_trainer_step_matches_torch_adamw_on_the_oracle).  Eager: two steps.
    graph=True: four, because the trainer runs its first two steps of a shape eagerly — steps 2 and 3 are the capture's
    replays, whose by-value arguments are frozen and whose masks move only through `step_dev`."""
    from mrmt3.trainer import Trainer
    mel, lab, _ = d_inputs
    m = _model("t5", torch.float32, dev)
    tr = Trainer(m, lr=1e-3, graph=graph)
    n = 4 if graph else 2
    losses = [float(tr.train_step(mel.to(dev), lab.to(dev)).item()) for _ in range(n)]
    torch.cuda.synchronize()
    captured = tr.graph_captured
    tr.close()
    print("graph=%s losses %s oracle %s" % (graph, losses, adamw_trajectory[:n]))
    assert captured == graph
    assert np.allclose(losses, adamw_trajectory[:n], rtol=0, atol=5e-5), (losses, adamw_trajectory[:n])


def test_accumulated_gradient_is_the_sum_over_the_micro_batch_salts(dev, d_inputs):
    """accumulate_grad_batches = 2, fp32, eager: after the cycle `flat.G` (before the 1/2 the optimizer applies) is the
    masked oracle's gradient of micro-batch 0 under salt 0 plus that of micro-batch 1 under salt 1, both at the initial
    weights: every tensor within rel-L2 1e-4."""
    from mrmt3.trainer import Trainer
    mel, lab, _ = d_inputs
    mel1, lab1, _ = _inputs(2, 256, 64, seed=71, mean_len=40)
    cfg = _cfg()
    m = _model("t5", torch.float32, dev)
    tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=2)
    l0 = float(tr.train_step(mel.to(dev), lab.to(dev)).item())
    l1 = float(tr.train_step(mel1.to(dev), lab1.to(dev)).item())
    torch.cuda.synchronize()
    assert tr.optimizer_steps == 1 and tr.pending_micro_batches == 0
    got = {k: m.flat.grad(k).detach().float().cpu().clone() for k in m.flat.shapes}
    tr.close()
    r0, _, g0 = oracle_grads(cfg, mel, lab, drop=DropPlan(P, step=0))
    r1, _, g1 = oracle_grads(cfg, mel1, lab1, drop=DropPlan(P, step=1))
    assert abs(l0 - r0) < 2e-5 and abs(l1 - r1) < 2e-5, (l0, r0, l1, r1)
    worst = (0.0, "")
    for k, g in got.items():
        rel = rel_l2(g, g0[k] + g1[k])
        worst = max(worst, (rel, k))
        assert rel < 1e-4, (k, rel)
    print("accumulated G: worst rel-L2 %.3e (%s)" % worst)
