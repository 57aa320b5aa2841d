"""Optimizer parameter groups on the MI355X: mrmt3_adamw_step / mrmt3_grad_norm over a range table alone, then the
trainer with frozen weights, no-decay sets and EMA weights — against tests/optim_groups_ref.py (torch.optim.AdamW with real
param groups, a float64 EMA loop), against the flat form of the same entry points bit for bit, eager against graph replay."""
import socket

import numpy as np
import pytest
import torch

from optim_groups_ref import TorchGroups, ema64, match, small_cfg

pytestmark = pytest.mark.gpu

N = 16384                   # elements of the kernel tests' buffer: 4 workgroups of the grouped step (1024 16-byte groups each)
# (begin, end, weight_decay, lr_scale): a 4-element range, one 4-element frozen gap, a range over several workgroups, a
# range ending at n
RANGES = [(0, 4, 0.01, 1.0), (8, 16, 0.0, 0.5), (1000, 11000, 0.05, 2.0), (N - 8, N, 0.01, 0.25)]
SENTINEL = {"p": 0x4B7FABCD, "m": 0x4B7F1234, "v": 0x4B7F5678, "ema": 0x4B7F9ABC, "g": 0x7FC00001}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mask(ranges, n, dev):
    m = torch.zeros(n, dtype=torch.bool, device=dev)
    for a, b, _, _ in ranges:
        m[a:b] = True
    return m


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _buffers(dev, n=N, ranges=RANGES, seed=0):
    """p, g, m, v, ema, shadow with random contents inside the ranges and a sentinel bit pattern (a NaN in g) outside."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    b = {k: torch.randn(n, device=dev, generator=gen) for k in ("p", "g", "m", "v", "ema")}
    b["v"] = b["v"].abs() * 1e-3
    frozen = ~_mask(ranges, n, dev)
    for k, bits in SENTINEL.items():
        _bits(b[k])[frozen] = bits
    b["s"] = b["p"].bfloat16()
    _bits(b["s"])[frozen] = 0x4B7F
    return b, frozen


def _table(dev, ranges=RANGES, n=N):
    from mrmt3 import lib
    return lib.OptRanges(ranges, n).to(dev)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True])
def test_grouped_step_equals_the_one_group_kernel_per_range_and_leaves_frozen_bits(dev, clipped):
    """Inside each range P, M, V and the bf16 shadow are bit-equal to the flat mrmt3_adamw_step (clipped: with stat_dev,
    coefficient 0.5 and a clamp) run on a copy of that range with the range's weight decay and lr * lr_scale; every element
    outside the ranges keeps its sentinel bits in p, m, v, shadow and ema; the EMA moved inside the ranges."""
    from mrmt3 import lib
    b, frozen = _buffers(dev)
    before = {k: t.clone() for k, t in b.items()}
    tab = _table(dev)
    assert tab.n_trainable == sum(r[1] - r[0] for r in RANGES)
    lr = torch.full((1,), 1e-2, device=dev)
    step = torch.full((1,), 6, device=dev, dtype=torch.int32)
    stat = torch.tensor([3.0, 0.5, 0.0, 0.0], device=dev) if clipped else None
    lib.adamw_step(b["p"], b["g"], b["m"], b["v"], lr, step, grad_scale=1.0 / 3, ranges=tab, ema=b["ema"], ema_decay=0.9,
                   stat=stat, clip_value=0.2 if clipped else 0.0, shadow=b["s"])
    torch.cuda.synchronize()
    assert int(step.item()) == 7
    for k in ("p", "m", "v", "ema", "s"):
        assert torch.equal(_bits(b[k])[frozen], _bits(before[k])[frozen]), k
    for a, e, wd, sc in RANGES:
        P, G, M, V = (before[k][a:e].clone() for k in ("p", "g", "m", "v"))
        S = torch.zeros(e - a, device=dev, dtype=torch.bfloat16)
        lr_r = lr * torch.tensor(sc, device=dev)                                  # the kernel's f32 product
        st = torch.full((1,), 6, device=dev, dtype=torch.int32)
        if clipped:
            lib.adamw_step(P, G, M, V, lr_r, st, weight_decay=wd, grad_scale=1.0 / 3, stat=stat, clip_value=0.2, shadow=S)
        else:
            lib.adamw_step(P, G, M, V, lr_r, st, weight_decay=wd, grad_scale=1.0 / 3, shadow=S)
        torch.cuda.synchronize()
        for got, want in ((b["p"], P), (b["m"], M), (b["v"], V), (b["s"], S)):
            assert torch.equal(_bits(got[a:e]), _bits(want)), (a, e)
        assert not torch.equal(P, before["p"][a:e])
        want_ema = before["ema"][a:e] + (torch.tensor(1.0, device=dev) - torch.tensor(0.9, device=dev)) * (P - before["ema"][a:e])
        assert torch.equal(b["ema"][a:e], want_ema), (a, e)
    # without an EMA buffer: the same P, and ema is not touched anywhere
    c = {k: t.clone() for k, t in before.items()}
    step.fill_(6)
    lib.adamw_step(c["p"], c["g"], c["m"], c["v"], lr, step, grad_scale=1.0 / 3, ranges=tab, stat=stat,
                   clip_value=0.2 if clipped else 0.0, shadow=c["s"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(c["p"]), _bits(b["p"])) and torch.equal(_bits(c["ema"]), _bits(before["ema"]))


def test_one_range_over_the_buffer_equals_the_one_group_step_and_norm_bitwise(dev):
    """The all-trainable table (what EMA alone installs) at a length that is no multiple of the workgroup's chunk."""
    from mrmt3 import lib
    n = 4 * 70001
    gen = torch.Generator(device=dev).manual_seed(9)
    p, g, m, v = (torch.randn(n, device=dev, generator=gen) for _ in range(4))
    v = v.abs() * 1e-3
    tab = lib.OptRanges([(0, n, 0.01, 1.0)], n).to(dev)
    lr = torch.full((1,), 1e-3, device=dev)
    out = []
    for grouped in (False, True):
        P, M, V, S = p.clone(), m.clone(), v.clone(), torch.zeros(n, device=dev, dtype=torch.bfloat16)
        step = torch.full((1,), 2, device=dev, dtype=torch.int32)
        if grouped:
            lib.adamw_step(P, g, M, V, lr, step, grad_scale=0.25, ranges=tab, shadow=S)
        else:
            lib.adamw_step(P, g, M, V, lr, step, grad_scale=0.25, shadow=S)
        out.append((P, M, V, S))
    torch.cuda.synchronize()
    for x, y in zip(*out):
        assert torch.equal(_bits(x), _bits(y))
    ws = lib.grad_norm_workspace(dev)
    s1, s2 = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
    sk = torch.zeros(1, device=dev, dtype=torch.int32)
    lib.grad_norm(g, 0.5, 1.0, False, ws, s1, sk)
    lib.grad_norm(g, 0.5, 1.0, False, ws, s2, sk, ranges=tab)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1), _bits(s2)) and float(s1[0]) > 0


def test_ema_after_eight_steps_against_float64(dev):
    """ema against the float64 recurrence over the GPU's own p trajectory.  Each step's f32 update rounds at relative 2^-24
    of max(|ema|, |p|) (the difference, the product with 1 - decay and the sum: the first two are scaled down by
    1 - decay), so after N steps |ema - ema64| <= N * 2^-23 * max|p|."""
    from mrmt3 import lib
    steps, decay = 8, 0.9
    b, frozen = _buffers(dev, seed=3)
    tab = _table(dev)
    lr = torch.full((1,), 1e-2, device=dev)
    step = torch.zeros(1, device=dev, dtype=torch.int32)
    ema0 = b["ema"].double().cpu().numpy()
    keep = ~frozen.cpu().numpy()
    traj = []
    gen = torch.Generator(device=dev).manual_seed(4)
    for _ in range(steps):
        b["g"][~frozen] = torch.randn(int((~frozen).sum()), device=dev, generator=gen)
        lib.adamw_step(b["p"], b["g"], b["m"], b["v"], lr, step, ranges=tab, ema=b["ema"], ema_decay=decay)
        torch.cuda.synchronize()
        traj.append(b["p"].double().cpu().numpy()[keep])
    want = ema64(traj, decay, ema0[keep])
    got = b["ema"].double().cpu().numpy()[keep]
    pmax = max(float(np.abs(t).max()) for t in traj + [ema0[keep]])
    bound = steps * 2.0 ** -23 * pmax
    err = float(np.abs(got - want).max())
    print("ema after %d steps: max|ema - ema64| = %.3e, bound %.3e (max|p| %.3f)" % (steps, err, bound, pmax))
    assert err <= bound
    assert float(np.abs(got - ema0[keep]).max()) > 0.1                           # the EMA really moved
    assert int(step.item()) == steps


def test_nonfinite_gradient_skips_everything_only_when_it_is_trainable(dev):
    """An inf in a trainable gradient under skip_nonfinite: the norm over the ranges is non-finite and the step changes
    nothing, the EMA included (step_dev still counts it).  The same inf in a FROZEN slot is never read: the norm is finite
    and the step proceeds."""
    from mrmt3 import lib
    tab = _table(dev)
    ws = lib.grad_norm_workspace(dev)
    lr = torch.full((1,), 1e-2, device=dev)
    for slot, skipped_want in ((2000, 1), (500, 0)):                             # 2000: inside range 2; 500: frozen
        b, frozen = _buffers(dev, seed=5)
        b["g"][frozen] = 0.0                                                     # (finite everywhere but the planted slot)
        assert bool(frozen[slot]) == (skipped_want == 0)
        b["g"][slot] = float("inf")
        before = {k: t.clone() for k, t in b.items()}
        stat, skipped = torch.zeros(4, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
        step = torch.full((1,), 3, device=dev, dtype=torch.int32)
        lib.grad_norm(b["g"], 0.5, 1.0, True, ws, stat, skipped, ranges=tab)
        lib.adamw_step(b["p"], b["g"], b["m"], b["v"], lr, step, grad_scale=0.5, ranges=tab, ema=b["ema"], ema_decay=0.99,
                       stat=stat, shadow=b["s"])
        torch.cuda.synchronize()
        st = stat.cpu().numpy()
        assert int(step.item()) == 4 and int(skipped.item()) == skipped_want
        if skipped_want:
            assert not np.isfinite(st[0]) and st[1] == 0.0 and st[2] == 1.0
            for k in ("p", "m", "v", "ema", "s"):
                assert torch.equal(_bits(b[k]), _bits(before[k])), k
        else:
            assert np.isfinite(st[0]) and st[0] > 0 and 0 < st[1] < 1 and st[2] == 0.0
            keep = ~frozen
            assert not torch.equal(b["p"][keep], before["p"][keep]) and bool(torch.isfinite(b["p"][keep]).all())
            assert not torch.equal(b["ema"][keep], before["ema"][keep])
            for k in ("p", "m", "v", "ema", "s"):
                assert torch.equal(_bits(b[k])[frozen], _bits(before[k])[frozen]), k


def _within_one_ulp(got, want):
    """The tolerance tests/test_grad_clip_gpu.py holds mrmt3_grad_norm to: the float64 norm rounded to f32, within 1 ulp."""
    got, want = np.float32(got), np.float32(want)
    return abs(float(got) - float(want)) <= float(np.spacing(want))


def test_norm_over_ranges_equals_float64_within_one_ulp(dev):
    """The edge-case table, then a buffer long enough for the four-strides-at-a-time loop of the fixed grid (more than
    3 x 2048 x 256 16-byte groups inside the ranges) with gaps; NaNs sit in every frozen slot, so a read outside the ranges
    would show.  Same bits on a second call."""
    from mrmt3 import lib
    stride = 2048 * 256 * 4
    big_n = 4 * stride + 4096
    big = [(0, stride - 4, 0.01, 1.0), (stride, 2 * stride + 1028, 0.0, 1.0), (2 * stride + 1032, big_n - 8, 0.01, 0.5),
           (big_n - 4, big_n, 0.01, 1.0)]
    ws = lib.grad_norm_workspace(dev)
    gen = torch.Generator(device=dev).manual_seed(6)
    for ranges, n, scale in ((RANGES, N, 1.0), (RANGES[:1], N, 0.5), (big, big_n, 1.0 / 3)):
        keep = _mask(ranges, n, dev)
        mag = torch.pow(10.0, torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * 9 - 6)
        sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
        g = (mag * sign).float()
        g[~keep] = float("nan")
        want = np.float32(float(g[keep].double().pow(2).sum().sqrt().item()) * float(np.float32(scale)))
        tab = lib.OptRanges(ranges, n).to(dev)
        got = []
        for _ in range(2):
            stat, skipped = torch.full((4,), -7.0, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
            lib.grad_norm(g, scale, float(want) / 2, False, ws, stat, skipped, ranges=tab)
            torch.cuda.synchronize()
            got.append(stat.cpu().numpy())
        print("n = %d, %d ranges: norm %.9g, float64 %.9g" % (n, len(ranges), got[0][0], want))
        assert _within_one_ulp(got[0][0], want), (got[0][0], want)
        assert got[0].tobytes() == got[1].tobytes() and got[0][1] < 1 and got[0][2] == 0 and got[0][3] == -7.0


# ---- 2. the trainer --------------------------------------------------------------------------------------------------
FROZEN = ["encoder.*"]
NO_DECAY = ["*layer_norm.weight"]


def _model(dtype, dev, **over):
    from models.t5 import T5ForConditionalGeneration
    return T5ForConditionalGeneration(small_cfg(**over), compute_dtype=dtype).load_golden().to(dev)


def _batch(dev, seed, B=2, L=32):
    from mrmt3.synthetic import synth_mel, synth_labels
    mel = torch.from_numpy(synth_mel(B, seed=seed + 1)).to(dev)
    lab = torch.from_numpy(synth_labels(B, L, full=False, seed=seed + 2, mean_len=20)).to(dev)
    return mel, lab


def _counts(fn):
    from mrmt3 import lib
    lib.dispatch_counts(reset=True)
    fn()
    torch.cuda.synchronize()
    return lib.dispatch_counts(reset=True)


def _wgrad_launches(c):
    return c["tn_f32"] + c["tn8"] + c["tn_tile"] + c["tn_group"]


def _oracle_grads(weights, cfg, mel, lab):
    """float64 autograd gradients of the oracle at `weights` {key: f32 tensor} (zeros where a tensor gets none)."""
    from oracle import t5_ref
    sd = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in weights.items()}
    loss = t5_ref.ce_loss(t5_ref.forward_logits(sd, cfg, mel.cpu().double(), lab.cpu()), lab.cpu())
    loss.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


def _rel_update(model, ref, p0, keys):
    """||P - P_ref|| / ||P_ref - P0|| over the tensors `keys`."""
    num = den = 0.0
    for k in keys:
        a, r = model.flat.master(k).detach().double().cpu(), ref.weights()[k].double()
        num += float((a - r).pow(2).sum())
        den += float((r - p0[k].double()).pow(2).sum())
    return (num / den) ** 0.5


def test_frozen_encoder_fp32_against_torch_param_groups(dev):
    """fp32 engine, p = 0, three steps, encoder frozen, norm weights without decay.  Frozen tensors keep their bits; the
    trainable ones follow torch.optim.AdamW with real param groups stepping on the oracle's float64 autograd gradients,
    within twice the deviation the all-trainable trainer shows against all-trainable torch AdamW on the same data (the
    pruned backward changes no arithmetic of the kept gradients: after step 1 they are bit-equal to the all-trainable
    step's); no attention backward runs for the encoder and its weight-gradient products are gone.
    Measured on the MI355X: all-trainable 1.425e-4, encoder frozen + no-decay norms 1.471e-4."""
    from mrmt3 import checkpoint as ck
    from mrmt3.trainer import Trainer
    torch.set_num_threads(8)
    cfg = small_cfg(dropout_rate=0.0)
    data = [_batch(dev, 10 * i) for i in range(3)]
    order = ck.reference_parameter_order(cfg, 0)
    dev_rel, counts, grads1 = {}, {}, {}
    for name, frozen, no_decay in (("all", None, None), ("frozen", FROZEN, NO_DECAY)):
        m = _model(torch.float32, dev, dropout_rate=0.0)
        p0 = {k: m.flat.master(k).detach().cpu().clone() for k in order}
        tr = Trainer(m, lr=1e-3, graph=False, frozen=frozen, no_decay=no_decay)
        ref = TorchGroups(p0, order, frozen=match(order, frozen), no_decay=match(order, no_decay), lr=1e-3)
        for i, (mel, lab) in enumerate(data):
            c = _counts(lambda: tr.train_step(mel, lab))
            if i == 0:
                counts[name] = c
                grads1[name] = m.flat.G.clone()
            ref.step(_oracle_grads(ref.weights(), cfg, mel, lab))
        keys = [k for k in order if k not in match(order, FROZEN)]           # the decoder side, in both runs
        dev_rel[name] = _rel_update(m, ref, p0, keys)
        if frozen:
            for k in match(order, frozen):
                assert torch.equal(_bits(m.flat.master(k)).cpu(), _bits(p0[k])), k
                assert not bool(m.flat.view(m.flat.M, k).any()) and not bool(m.flat.view(m.flat.V, k).any()), k
            for k in keys:
                assert torch.equal(m.flat.view(grads1["frozen"], k), m.flat.view(grads1["all"], k)), k
            assert tr.groups_on and len(m.flat.opt_ranges) < len(keys)
    print("fp32, 3 steps, rel-L2 of the update against torch AdamW on the oracle's gradients: all-trainable %.3e, "
          "encoder frozen + no-decay norms %.3e" % (dev_rel["all"], dev_rel["frozen"]))
    assert dev_rel["frozen"] <= 2 * dev_rel["all"]
    n_enc = cfg["num_layers"]
    # attn_f32 counts forward and backward launches: the frozen step lacks exactly the encoder's backward ones
    assert counts["all"]["attn_f32"] - counts["frozen"]["attn_f32"] == n_enc
    assert counts["frozen"]["attn_f32"] == n_enc + 2 * 2 * cfg["num_decoder_layers"]
    # weight-gradient products: 4 per encoder layer + proj are gone (at these tiny row counts none takes the grouped
    # launch, whose pruning test_frozen_step_replays_bitwise... shows at a size where it does)
    assert _wgrad_launches(counts["all"]) - _wgrad_launches(counts["frozen"]) == 4 * n_enc + 1


def test_frozen_step_replays_bitwise_and_prunes_the_grouped_launch(dev):
    """bf16 engine, dropout on, encoder frozen + no-decay norms + an EMA, 4 x 256 = 1024 decoder and encoder rows — the
    fewest at which the grouped weight-gradient launch takes a product (below, every gradient goes one by one): the replayed steps equal the eager trainer's bit for bit (P, M, V, shadow, EMA), the
    frozen tensors never change, the grouped launch plans fewer items than the all-trainable step's and the attention
    backward runs for the decoder's sites only."""
    from mrmt3.trainer import Trainer
    data = [_batch(dev, 100 + 10 * i, B=4, L=256) for i in range(5)]
    runs, items = {}, {}
    for use_graph in (False, True):
        m = _model(torch.bfloat16, dev)
        p0 = m.flat.P.clone()
        tr = Trainer(m, lr=1e-3, graph=use_graph, frozen=FROZEN, no_decay=NO_DECAY, ema_decay=0.9)
        seen = []
        for i, x in enumerate(data):
            c = _counts(lambda: tr.train_step(*x))
            if not use_graph and i == 0:
                n_dec = m.cfg["num_decoder_layers"]
                assert c["attn_bwd"] + c["attn_bwd_onepass"] + c["attn_bwd_varlen"] == 2 * n_dec, c
                assert c["tn_group"] >= 1
                items["frozen"] = (m.engine.tn_group.last_info.n_items, _wgrad_launches(c))
            seen.append(m.flat.P.clone())
        assert tr.graph_captured == use_graph
        frozen = ~_mask([(a, b, 0, 0) for a, b in m.flat.trainable_spans()], m.flat.numel, dev)
        assert int(frozen.sum()) > 0 and torch.equal(_bits(m.flat.P)[frozen], _bits(p0)[frozen])
        assert torch.equal(_bits(m.flat.E)[frozen], _bits(p0)[frozen]) and not torch.equal(m.flat.E[~frozen], m.flat.P[~frozen])
        assert not torch.equal(m.flat.P[~frozen], p0[~frozen])
        runs[use_graph] = seen + [m.flat.M.clone(), m.flat.V.clone(), m.flat.S.clone(), m.flat.E.clone()]
        tr.close()
    for x, y in zip(runs[False], runs[True]):
        assert torch.equal(_bits(x), _bits(y))
    m = _model(torch.bfloat16, dev)
    tr = Trainer(m, lr=1e-3, graph=False)
    c = _counts(lambda: tr.train_step(*data[0]))
    items["all"] = (m.engine.tn_group.last_info.n_items, _wgrad_launches(c))
    print("grouped weight-gradient items / weight-gradient launches: all-trainable %s, encoder frozen %s" % (items["all"], items["frozen"]))
    assert items["frozen"][0] < items["all"][0] and items["frozen"][1] <= items["all"][1]
    assert c["attn_bwd"] + c["attn_bwd_onepass"] + c["attn_bwd_varlen"] == 2 * m.cfg["num_decoder_layers"] + m.cfg["num_layers"]


def _drive(tr, m, ref, order, data, p_bound, gmax):
    """Run the steps; after each, the reference steps on the GPU's own gradients and P is compared to it.  gmax collects
    each tensor's largest |gradient| so far."""
    for x in data:
        tr.train_step(*x)
        torch.cuda.synchronize()
        for k in order:
            gmax[k] = max(gmax.get(k, 0.0), float(m.flat.grad(k).abs().max()))
        ref.step({k: m.flat.grad(k) for k in order})
        worst = max(float((m.flat.master(k).cpu() - ref.weights()[k]).abs().max()) for k in order)
        assert worst <= p_bound(), (tr.host_step, worst, p_bound())


def test_set_frozen_recaptures_and_thawed_moments_continue(dev):
    """bf16 engine, graph replay, dropout 0: three steps with everything trainable, set_frozen(encoder) for three, thawed
    for three.  Each change drops the captured graph and the step is captured again; while frozen the encoder keeps its
    weights AND its moments, and after the thaw they continue from there — P, M and V follow torch.optim.AdamW with the
    same param groups stepping on the GPU's own gradients (its per-tensor step count set to the optimizer's global one,
    which is what the flat optimizer's single counter means for bias correction).
    Bound on P: both sides round p a few times per step at 2^-24 relative (decay product, quotient, product, difference):
    8 * 2^-24 * max|p| per step."""
    from mrmt3 import checkpoint as ck
    from mrmt3.trainer import Trainer
    cfg = small_cfg(dropout_rate=0.0)
    order = ck.reference_parameter_order(cfg, 0)
    data = [_batch(dev, 200 + 10 * i) for i in range(9)]
    m = _model(torch.bfloat16, dev, dropout_rate=0.0)
    p0 = {k: m.flat.master(k).detach().cpu().clone() for k in order}
    pmax = float(m.flat.P.abs().max())
    tr = Trainer(m, lr=1e-3, graph=True, no_decay=NO_DECAY)
    ref = TorchGroups(p0, order, no_decay=match(order, NO_DECAY), lr=1e-3)
    bound = lambda: 8 * 2.0 ** -24 * (pmax + 0.01) * tr.host_step
    gmax = {}
    _drive(tr, m, ref, order, data[:3], bound, gmax)
    assert tr.graph_captured
    enc = sorted(match(order, FROZEN))
    tr.set_frozen(FROZEN)
    assert not tr.graph_captured
    ref.set_frozen(match(order, FROZEN))
    held = {k: (m.flat.master(k).clone(), m.flat.view(m.flat.M, k).clone(), m.flat.view(m.flat.V, k).clone()) for k in enc}
    assert all(bool(v[1].any()) for v in held.values())
    _drive(tr, m, ref, order, data[3:6], bound, gmax)
    assert tr.graph_captured
    for k in enc:
        for got, want in zip((m.flat.master(k), m.flat.view(m.flat.M, k), m.flat.view(m.flat.V, k)), held[k]):
            assert torch.equal(_bits(got), _bits(want)), k
    tr.set_frozen(None)
    assert not tr.graph_captured and not m.flat.frozen
    ref.set_frozen(())
    for p, s in ref.opt.state.items():
        s["step"] = torch.tensor(float(tr.host_step))
    _drive(tr, m, ref, order, data[6:], bound, gmax)
    assert tr.graph_captured and tr.host_step == 9
    for k in enc:
        assert not torch.equal(m.flat.master(k), held[k][0]), k
    for k in order:
        st = ref.opt.state[ref.p[k]]
        # a moment is a signed sum of terms as large as the tensor's largest |g| (|g|^2 for V): each of the nine steps rounds
        # it a few times at 2^-24 of that size on either side, whatever is left after cancellation — 9 * 8 * 2^-24 * max|g|
        tol = 9 * 8 * 2.0 ** -24 * gmax[k]
        assert float((m.flat.view(m.flat.M, k).cpu() - st["exp_avg"]).abs().max()) <= tol, k
        assert float((m.flat.view(m.flat.V, k).cpu() - st["exp_avg_sq"]).abs().max()) <= tol * gmax[k], k
    tr.close()


def test_ema_weights_context_swaps_and_restores_bitwise(dev):
    """bf16, dropout on.  Inside `with trainer.ema_weights()` eval_loss is that of a fresh model loaded from
    ema_state_dict(), bit for bit, and training raises; after it P and the shadow are bit-equal to before, and the next
    train_step equals the step of a twin trainer that never entered the context."""
    from mrmt3.trainer import Trainer
    data = [_batch(dev, 300 + 10 * i) for i in range(4)]
    ev = _batch(dev, 390)
    out = {}
    for enter in (True, False):
        m = _model(torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=False, ema_decay=0.9, no_decay=NO_DECAY)
        for x in data[:3]:
            tr.train_step(*x)
        torch.cuda.synchronize()
        if enter:
            plain = tr.eval_loss(*ev).clone()
            before = (m.flat.P.clone(), m.flat.S.clone(), m.flat.ST.clone())
            sd = tr.ema_state_dict()
            with tr.ema_weights():
                inside = tr.eval_loss(*ev).clone()
                score_in = m.score(*ev).clone()
                assert torch.equal(m.flat.P, m.flat.E)
                with pytest.raises(RuntimeError, match="ema_weights"):
                    tr.train_step(*data[3])
                with pytest.raises(RuntimeError, match="ema_weights"):
                    tr.set_frozen(FROZEN)
            torch.cuda.synchronize()
            for got, want in zip((m.flat.P, m.flat.S, m.flat.ST), before):
                assert torch.equal(_bits(got), _bits(want))
            assert torch.equal(tr.eval_loss(*ev), plain)
            fresh = _model(torch.bfloat16, dev)
            fresh.load_state_dict(sd)
            ftr = Trainer(fresh, lr=1e-3, graph=False)
            want_in = ftr.eval_loss(*ev)
            torch.cuda.synchronize()
            print("eval loss: training weights %.6f, EMA weights %.6f" % (float(plain), float(inside)))
            assert torch.equal(inside, want_in) and not torch.equal(inside, plain)
            assert torch.equal(score_in, fresh.score(*ev))
            assert set(sd) == set(m.state_dict()) and torch.equal(sd["encoder.embed_tokens.weight"], sd["proj.weight"])
        tr.train_step(*data[3])
        torch.cuda.synchronize()
        out[enter] = [t.clone() for t in (m.flat.P, m.flat.M, m.flat.V, m.flat.S, m.flat.E)]
    for x, y in zip(out[True], out[False]):
        assert torch.equal(_bits(x), _bits(y))
    with pytest.raises(RuntimeError, match="ema_decay"):
        Trainer(_model(torch.bfloat16, dev), graph=False).ema_state_dict()


def test_forced_collectives_exchange_trainable_slices_only(dev, monkeypatch):
    """World size 1 with the collectives forced: every slice a bucket sends lies inside trainable tensors, the encoder's
    buckets are gone, and the step equals the un-bucketed one bit for bit."""
    import torch.distributed as dist
    from mrmt3.trainer import Trainer
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    data = [_batch(dev, 400 + 10 * i) for i in range(2)]
    out = {}
    for force in (True, False):
        if force:
            monkeypatch.setenv("MRMT3_DDP_FORCE_COLLECTIVES", "1")
            dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
        try:
            m = _model(torch.bfloat16, dev, dropout_rate=0.0)
            tr = Trainer(m, lr=1e-3, graph=False, frozen=FROZEN + ["decoder.block.0.layer.0.layer_norm.weight"], layers_per_bucket=1)
            assert tr.buckets.active == force
            sent = []
            orig = tr.buckets._all_reduce
            tr.buckets._all_reduce = lambda t, stream=None: (sent.append(((t.data_ptr() - m.flat.G.data_ptr()) // 4, t.numel())),
                                                             orig(t, stream))[1]
            for x in data:
                tr.train_step(*x)
            torch.cuda.synchronize()
            if force:
                spans = m.flat.trainable_spans()
                assert len(tr.buckets.buckets) < len(tr.buckets._all_buckets)
                assert any(len(b["slices"]) == 2 for b in tr.buckets.buckets)          # the bucket around the frozen norm weight
                assert not any(b["trigger"][0] == "encoder" for b in tr.buckets.buckets)
                assert sent and all(any(a <= off and off + n <= b for a, b in spans) for off, n in sent), sent
                assert sum(n for _, n in sent) == 2 * sum(b - a for a, b in spans)       # every trainable element, once per step
            else:
                assert not sent
            out[force] = [t.clone() for t in (m.flat.P, m.flat.M, m.flat.V)]
            tr.close()
        finally:
            if force:
                dist.destroy_process_group()
                monkeypatch.delenv("MRMT3_DDP_FORCE_COLLECTIVES")
    for x, y in zip(out[True], out[False]):
        assert torch.equal(_bits(x), _bits(y))


def test_checkpoint_resume_restores_groups_and_ema(dev, tmp_path):
    """save_checkpoint / resume carry the EMA weights, the patterns and the grouped moments: a resumed trainer built WITHOUT
    the options continues bit for bit with the run that never stopped (dropout off)."""
    from mrmt3.trainer import Trainer
    data = [_batch(dev, 500 + 10 * i) for i in range(3)]
    m = _model(torch.bfloat16, dev, dropout_rate=0.0)
    tr = Trainer(m, lr=1e-3, graph=False, frozen=FROZEN, no_decay=NO_DECAY, ema_decay=0.9)
    for x in data[:2]:
        tr.train_step(*x)
    path = str(tmp_path / "g.ckpt")
    tr.save_checkpoint(path)
    tr.train_step(*data[2])
    torch.cuda.synchronize()
    m2 = _model(torch.bfloat16, dev, dropout_rate=0.0)
    tr2 = Trainer(m2, lr=1e-3, graph=False)
    assert tr2.resume(path) == 2 and tr2.ema_decay == 0.9 and tr2.groups.patterns["frozen"] == FROZEN
    assert m2.flat.frozen == m.flat.frozen and m2.flat.opt_ranges.ranges == m.flat.opt_ranges.ranges
    tr2.train_step(*data[2])
    torch.cuda.synchronize()
    for a, b in ((m.flat.P, m2.flat.P), (m.flat.E, m2.flat.E)):
        assert torch.equal(_bits(a), _bits(b))
    keep = _mask([(a, b, 0, 0) for a, b in m.flat.trainable_spans()], m.flat.numel, dev)
    assert torch.equal(m.flat.M[keep], m2.flat.M[keep]) and torch.equal(m.flat.V[keep], m2.flat.V[keep])


def test_default_trainer_is_the_one_group_step_of_before(dev, monkeypatch):
    """None of the options: the norm is never called, no range table is built, lib.adamw_step gets no `stat`, `ranges` or
    `ema`, the launches per family are those of the model's
    structure (what the step launched before), and two steps give exactly the weights of a by-hand loop of lib.adamw_step
    over the same gradients."""
    from mrmt3 import lib
    from mrmt3.trainer import Trainer

    def boom(*a, **k):
        raise AssertionError("no option is on: no grouped launch, no range table")
    for name in ("grad_norm", "grad_norm_workspace", "OptRanges"):
        monkeypatch.setattr(lib, name, boom)
    plain_step, plain_calls = lib.adamw_step, []

    def spy(*a, stat=None, ranges=None, ema=None, **k):
        assert stat is None and ranges is None and ema is None and len(a) <= 12, "no option is on: the plain step"
        plain_calls.append(1)
        return plain_step(*a, **k)
    monkeypatch.setattr(lib, "adamw_step", spy)
    data = [_batch(dev, 600 + 10 * i) for i in range(2)]
    m = _model(torch.bfloat16, dev)
    tr = Trainer(m, lr=1e-3, graph=False)
    assert not tr.groups_on and m.flat.E is None and not m.flat.frozen
    P, M, V = m.flat.P.clone(), torch.zeros_like(m.flat.P), torch.zeros_like(m.flat.P)
    S = torch.zeros(m.flat.numel, device=dev, dtype=torch.bfloat16)
    lr, step = torch.full((1,), 1e-3, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    n_enc, n_dec = m.cfg["num_layers"], m.cfg["num_decoder_layers"]
    for x in data:
        c = _counts(lambda: tr.train_step(*x))
        assert _wgrad_launches(c) == 4 * n_enc + 1 + 7 * n_dec + 1, c              # every weight gradient, one launch each
        assert c["attn_bwd"] + c["attn_bwd_onepass"] + c["attn_bwd_varlen"] == n_enc + 2 * n_dec, c
        assert c["attn_fwd"] + c["attn_fwd_varlen"] == n_enc + 2 * n_dec, c
        lib.adamw_step(P, m.flat.G, M, V, lr, step, shadow=S)
    torch.cuda.synchronize()
    assert len(plain_calls) == 2 * len(data)                                       # the trainer's and the by-hand loop's
    for got, want in ((m.flat.P, P), (m.flat.M, M), (m.flat.V, V), (m.flat.S, S)):
        assert torch.equal(_bits(got), _bits(want))


def test_train_py_runs_with_the_group_keys_and_exports_the_ema(dev, tmp_path, monkeypatch, capsys):
    """train.py end to end on synthetic batches with +freeze / +no_decay / +ema_decay: the trainer gets the options, the run
    writes last_ema.pt (the EMA weights, a bare state dict that differs from last.pt only in trainable tensors) and a .ckpt
    that carries the patterns; +export_weights=ema makes last.pt the EMA weights."""
    import os
    import train
    from mrmt3 import checkpoint as ck
    from mrmt3 import trainer as trainer_mod
    from test_config_cpu import MODEL
    from test_grad_clip_gpu import TOP
    (tmp_path / "cfg" / "model").mkdir(parents=True)
    (tmp_path / "cfg" / "dataset").mkdir()
    (tmp_path / "cfg" / "config.yaml").write_text(TOP)
    (tmp_path / "cfg" / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    made, orig_init = [], trainer_mod.Trainer.__init__

    def init(self, *a, **k):
        made.append(self)
        orig_init(self, *a, **k)

    monkeypatch.setattr(trainer_mod.Trainer, "__init__", init)
    base = ["--config-dir", str(tmp_path / "cfg"), "--config-name", "config", "+synthetic=True", f"+output_dir={tmp_path / 'out'}",
            "+max_steps=3", '+freeze=["encoder.*"]', '+no_decay=["*layer_norm.weight"]', "+ema_decay=0.9"]
    train.main(base)
    tr = made[-1]
    assert tr.groups.patterns["frozen"] == ["encoder.*"] and tr.groups.patterns["no_decay"] == ["*layer_norm.weight"]
    assert tr.ema_decay == 0.9 and tr.groups_on and "proj.weight" in tr.flat.frozen
    out = tmp_path / "out" / "MT3Net_Slakh" / "version_0" / "checkpoints"
    last, ema = torch.load(out / "last.pt"), torch.load(out / "last_ema.pt")
    assert set(last) == set(ema)
    assert torch.equal(last["encoder.block.0.layer.0.SelfAttention.q.weight"], ema["encoder.block.0.layer.0.SelfAttention.q.weight"])
    assert not torch.equal(last["lm_head.weight"], ema["lm_head.weight"])
    blob = ck.read_checkpoint(str(out / "last.ckpt"))
    assert blob["extra"]["groups"]["frozen"] == ["encoder.*"] and blob["extra"]["groups"]["ema_decay"] == 0.9
    assert torch.equal(blob["extra"]["ema"]["lm_head.weight"], ema["lm_head.weight"])
    assert len(blob["optimizer"]["param_groups"]) == 2
    train.main(base + ["+export_weights=ema"])
    last2 = torch.load(out / "last.pt")
    assert torch.equal(last2["lm_head.weight"], ema["lm_head.weight"])              # the same seeded run: the same EMA
    with pytest.raises(ValueError, match="nothing_matches"):
        train.main(base[:-3] + ['+freeze=["nothing_matches*"]'])
    capsys.readouterr()
