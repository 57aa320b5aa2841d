"""Gradient clipping by global norm / by value, the logged gradient norm and the non-finite guard of the trainer
(`Trainer(gradient_clip_val=, gradient_clip_algorithm=, skip_nonfinite=, track_grad_norm=)`, mrmt3_grad_norm +
mrmt3_adamw_step with `stat_dev`) on the MI355X: the norm kernel against float64, the clipped AdamW step against float64, the
unclipped step's bits, graph replay against eager launches, accumulation, two ranks, skipped steps, train.py's log lines."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_grad_accum_gpu import _adamw64, _f64, _free_port, _micro, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _norm64(g, scale):
    """float32(sqrt(sum(g.double()^2)) * scale) with the sum taken by torch in float64; scale is the f32 the ABI receives."""
    return np.float32(float(g.double().pow(2).sum().sqrt().item()) * float(np.float32(scale)))


def _run_norm(g, scale, max_norm=0.0, skip=False, skipped=None):
    from mrmt3 import lib
    ws = lib.grad_norm_workspace(g.device)
    stat = torch.full((4,), -7.0, device=g.device)
    skipped = torch.zeros(1, device=g.device, dtype=torch.int32) if skipped is None else skipped
    lib.grad_norm(g, scale, max_norm, skip, ws, stat, skipped)
    torch.cuda.synchronize()
    return stat.cpu().numpy(), int(skipped.item())


def _within_one_ulp(got, want):
    got, want = np.float32(got), np.float32(want)
    return abs(float(got) - float(want)) <= float(np.spacing(want))


def _check_moments(flat, g64):
    """M and V after the FIRST f32 AdamW step against float64.  The kernel (like adamw_kernel) forms 1 - beta from the f32
    betas, and 1 - f32(0.999) is 1.3e-5 away from 0.001, so the float64 side takes the f32-rounded betas.  What is left: the
    f32 roundings of g * scale * coef, of the coefficient itself and of the two or three products per moment, each 2^-24 =
    6e-8 relative, about ten in all on V (which squares the gradient): 2e-6 relative."""
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert np.allclose(_f64(flat.M), (1.0 - b1) * g64, rtol=2e-6, atol=1e-30)
    assert np.allclose(_f64(flat.V), (1.0 - b2) * g64 * g64, rtol=2e-6, atol=1e-37)


# ---- 1. the norm kernel --------------------------------------------------------------------------------------------
def test_norm_kernel_equals_float64_within_one_ulp_and_is_deterministic(dev):
    """Random magnitudes over 1e-6 .. 1e3 at the model's size and at lengths around the fixed grid's stride (2048 x 256
    lanes x 4 floats = 2 097 152; the main loop takes four strides at a time), then a real gradient: stat[0] is the float64
    norm rounded to f32 within 1 ulp (the kernel accumulates in f64), the same bits on a second call, coef and skip as
    specified."""
    from mrmt3.trainer import Trainer
    gen = torch.Generator(device=dev).manual_seed(5)
    stride = 2048 * 256 * 4
    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    numel = m.flat.numel
    for n, scale in ((4, 1.0), (1028, 0.5), (stride - 4, 1.0), (stride + 4, 0.25), (4 * stride, 1.0), (5 * stride + 1028, 1.0 / 3),
                     (numel, 0.5)):
        mag = torch.pow(10.0, torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * 9 - 6)
        sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
        g = (mag * sign).float()
        want = _norm64(g, scale)
        s1, k1 = _run_norm(g, scale, max_norm=float(want) / 2)
        s2, _ = _run_norm(g, scale, max_norm=float(want) / 2)
        print("n = %d: norm %.9g, float64 %.9g" % (n, s1[0], want))
        assert _within_one_ulp(s1[0], want), (n, s1[0], want)
        assert s1[:3].tobytes() == s2[:3].tobytes()
        coef = np.float32(np.float32(float(want) / 2) / (s1[0] + np.float32(1e-6)))
        assert s1[1] == min(np.float32(1), coef) and s1[1] < 1 and s1[2] == 0 and k1 == 0 and s1[3] == -7.0
        s3, _ = _run_norm(g, scale, max_norm=0.0)
        assert s3[0] == s1[0] and s3[1] == 1.0 and s3[2] == 0
        s4, _ = _run_norm(g, scale, max_norm=float(want) * 4)
        assert s4[1] == 1.0
    tr = Trainer(m, lr=1e-3, graph=False, track_grad_norm=True)
    tr.train_step(*_micro(dev, B=1, L=128, seed=3))
    torch.cuda.synchronize()
    want = _norm64(m.flat.G, 1.0)
    got = float(tr.last_grad_norm.item())
    print("real gradient: norm %.9g, float64 %.9g" % (got, want))
    assert want > 0 and _within_one_ulp(got, want), (got, want)
    s, _ = _run_norm(m.flat.G, 1.0)
    assert np.float32(got) == s[0]
    assert tr.skipped_steps == 0


def test_norm_kernel_argument_errors(dev):
    from mrmt3 import lib
    g = torch.zeros(1024, device=dev)
    stat, skipped = torch.zeros(4, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    ws = lib.grad_norm_workspace(dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        lib.grad_norm(g[:1022], 1.0, 0.0, False, ws, stat, skipped)
    with pytest.raises(RuntimeError, match="workspace"):
        lib.grad_norm(g, 1.0, 0.0, False, ws[:64], stat, skipped)
    s, _ = _run_norm(g, 1.0, max_norm=1.0)              # an all-zero gradient: norm 0, coef clamps to 1
    assert s[0] == 0 and s[1] == 1 and s[2] == 0


# ---- 2. clip coefficient and AdamW ---------------------------------------------------------------------------------
def test_clipped_step_equals_float64_adamw_by_norm_and_by_value(dev):
    """fp32 engine, p = 0, eager: with gradient_clip_val = half the measured norm the parameters are one float64 AdamW step
    on G * coef64 (max-abs < 1e-6 at lr 1e-3, the unclipped step's bound), the moments follow, last_grad_norm is the norm
    BEFORE clipping; with algorithm "value" the gradient is np.clip'ed instead."""
    from mrmt3.trainer import Trainer
    batch = _micro(dev, B=1, L=192, seed=11)
    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    p0 = _f64(m.flat.P)
    tr = Trainer(m, lr=1e-3, graph=False, track_grad_norm=True)
    tr.train_step(*batch)
    torch.cuda.synchronize()
    norm0 = float(tr.last_grad_norm.item())
    gmax = float(m.flat.G.abs().max().item())
    assert np.isfinite(norm0) and norm0 > 0 and gmax > 0
    p64, _, _ = _adamw64(p0, _f64(m.flat.G), 0.0, 0.0, lr=1e-3, step=1)       # tracking alone: the unclipped step
    assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6

    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    tr = Trainer(m, lr=1e-3, graph=False, gradient_clip_val=norm0 / 2)
    tr.train_step(*batch)
    torch.cuda.synchronize()
    g = _f64(m.flat.G)
    n64 = float(np.sqrt((g * g).sum()))
    coef64 = (norm0 / 2) / (n64 + 1e-6)
    assert 0.45 < coef64 < 0.55
    assert _within_one_ulp(tr.last_grad_norm.item(), np.float32(n64))          # the pre-clip norm
    assert abs(float(tr._clip_stat[1].item()) - coef64) < 1e-6
    p64, _, _ = _adamw64(p0, g * coef64, 0.0, 0.0, lr=1e-3, step=1)
    print("norm: max|P - float64| = %.3e" % np.abs(_f64(m.flat.P) - p64).max())
    # After the FIRST AdamW step P hardly depends on the gradient's scale (m / sqrt(v) = sign(g) up to eps), so this bound
    # alone would pass with a wrong coefficient: what pins coef (and the clamp below) is the _clip_stat[1] comparison above
    # and the moments check that follows.  Keep them.
    assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6
    _check_moments(m.flat, g * coef64)
    assert int(tr.step_dev.item()) == 1 and tr.skipped_steps == 0

    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    cv = gmax / 8
    tr = Trainer(m, lr=1e-3, graph=False, gradient_clip_val=cv, gradient_clip_algorithm="value")
    tr.train_step(*batch)
    torch.cuda.synchronize()
    g = _f64(m.flat.G)
    cv32 = float(np.float32(cv))
    assert (np.abs(g) > cv32).sum() > 0
    assert _within_one_ulp(tr.last_grad_norm.item(), np.float32(np.sqrt((g * g).sum())))
    assert float(tr._clip_stat[1].item()) == 1.0
    p64, _, _ = _adamw64(p0, np.clip(g, -cv32, cv32), 0.0, 0.0, lr=1e-3, step=1)
    print("value: max|P - float64| = %.3e" % np.abs(_f64(m.flat.P) - p64).max())
    assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6
    _check_moments(m.flat, np.clip(g, -cv32, cv32))
    assert float(m.flat.M.abs().max().item()) <= 0.1 * cv32 * (1 + 1e-6)       # no moment saw more than the clamp


# ---- 3. neutrality -------------------------------------------------------------------------------------------------
def test_coefficient_one_is_the_unclipped_step_bit_for_bit(dev, monkeypatch):
    """bf16, dropout on, three steps: gradient_clip_val = 1e30 (coef exactly 1) leaves P, M, V and the bf16 shadow bit-equal
    to a trainer built without any of the options — and that trainer never calls the norm entry points, builds no range
    table, and calls lib.adamw_step without `stat`, `ranges` or `ema`."""
    from mrmt3 import lib
    from mrmt3.trainer import Trainer
    data = [_micro(dev, B=2, L=128, seed=20 + i) for i in range(3)]
    runs = {}
    for clip in (1e30, None):
        m = _model("t5", torch.bfloat16, dev)
        if clip is None:
            def boom(*a, **k):
                raise AssertionError("the feature is off: no norm / clipped launch may be issued")
            plain_step, plain_calls = lib.adamw_step, []

            def spy(*a, stat=None, ranges=None, ema=None, **k):
                assert stat is None and ranges is None and ema is None and len(a) <= 12, "the feature is off: the plain step"
                plain_calls.append(1)
                return plain_step(*a, **k)
            for name in ("grad_norm", "grad_norm_workspace", "OptRanges"):
                monkeypatch.setattr(lib, name, boom)
            monkeypatch.setattr(lib, "adamw_step", spy)
        tr = Trainer(m, lr=1e-3, graph=False, gradient_clip_val=clip)
        assert tr.clip_on == (clip is not None)
        for x in data:
            tr.train_step(*x)
        torch.cuda.synchronize()
        if clip is None:
            assert tr.last_grad_norm is None and tr.skipped_steps == 0 and len(plain_calls) == len(data)
        else:
            assert float(tr._clip_stat[1].item()) == 1.0 and float(tr.last_grad_norm.item()) > 0
        runs[clip] = [t.clone() for t in (m.flat.P, m.flat.M, m.flat.V, m.flat.S)]
    for x, y in zip(runs[1e30], runs[None]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("scale", [0.25, 1.0 / 3.0])
def test_abi_clipped_step_with_coefficient_one_equals_adamw_step_bitwise(dev, scale):
    """adamw_step(stat=[., 1, 0]) (adamw_kernel<true>) against adamw_step() (adamw_kernel<false>).  Also with an inexact grad_scale (1/3: three micro-batches or ranks): optim.hip is compiled with fp contract off, so
    neither kernel fuses g * scale into the next operation and the extra `* 1.0f` changes no bit."""
    from mrmt3 import lib
    n = 4 * 70001
    gen = torch.Generator(device=dev).manual_seed(9)
    p, g, m, v = (torch.randn(n, device=dev, generator=gen) for _ in range(4))
    v = v.abs() * 1e-3
    lr = torch.full((1,), 1e-3, device=dev)
    out = []
    for clipped in (False, True):
        P, M, V = p.clone(), m.clone(), v.clone()
        S = torch.zeros(n, device=dev, dtype=torch.bfloat16)
        step = torch.full((1,), 6, device=dev, dtype=torch.int32)
        if clipped:
            stat = torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev)
            lib.adamw_step(P, g, M, V, lr, step, grad_scale=scale, stat=stat, clip_value=0.0, shadow=S)
        else:
            lib.adamw_step(P, g, M, V, lr, step, grad_scale=scale, shadow=S)
        torch.cuda.synchronize()
        assert int(step.item()) == 7
        out.append((P, M, V, S))
    for x, y in zip(*out):
        assert torch.equal(x, y)


# ---- 4. replay = eager ---------------------------------------------------------------------------------------------
def test_replayed_clipped_step_equals_eager_bitwise_with_dropout(dev):
    """bf16, dropout 0.1, clipping active (coef < 1 in every step): two eager warm-up steps, the capture, then replays; the
    parameters after each of the five steps are bit-equal between the graph trainer and the eager trainer, and so are the
    norms: the replayed tail reads this step's coefficient from device memory."""
    from mrmt3.trainer import Trainer
    data = [_micro(dev, B=2, L=192, seed=40 + i, mean_len=60) for i in range(5)]
    runs = {}
    for use_graph in (False, True):
        m = _model("t5", torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=use_graph, gradient_clip_val=0.05)
        seen = []
        for x in data:
            tr.train_step(*x)
            torch.cuda.synchronize()
            seen.append((m.flat.P.clone(), tr._clip_stat.clone()))
        assert tr.graph_captured == use_graph
        assert all(float(s[1]) < 1.0 and float(s[2]) == 0.0 for _, s in seen), [s.tolist() for _, s in seen]
        assert int(tr.step_dev.item()) == 5 and tr.skipped_steps == 0
        runs[use_graph] = seen + [(m.flat.M.clone(), m.flat.V.clone())]
        tr.close()
    for (pe, se), (pg, sg) in zip(runs[False][:5], runs[True][:5]):
        assert torch.equal(pe, pg) and torch.equal(se, sg)
    assert torch.equal(runs[False][5][0], runs[True][5][0]) and torch.equal(runs[False][5][1], runs[True][5][1])
    norms = [float(s[0]) for _, s in runs[True][:5]]
    assert len(set(norms)) == 5, norms                       # every replay measured its own gradient


# ---- 5. accumulation -----------------------------------------------------------------------------------------------
def test_accumulated_clipped_step_and_partial_cycle_equal_float64(dev):
    """fp32, p = 0, eager.  N = 2: the update is float64 AdamW on (G / 2) * coef64 with coef64 from the norm of G / 2.
    N = 4 with two micro-batches and finish_accumulation(): the same on G / 4."""
    from mrmt3.trainer import Trainer
    micro = [_micro(dev, B=1, L=192, seed=60), _micro(dev, B=1, L=192, seed=70, mean_len=120)]
    for n_acc, finish in ((2, False), (4, True)):
        m = _model("t5", torch.float32, dev, dropout_rate=0.0)
        p0 = _f64(m.flat.P)
        tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=n_acc, gradient_clip_val=0.02)
        for x in micro:
            tr.train_step(*x)
        if finish:
            torch.cuda.synchronize()
            assert tr.pending_micro_batches == 2 and np.array_equal(_f64(m.flat.P), p0)
            assert tr.finish_accumulation()
        torch.cuda.synchronize()
        assert tr.optimizer_steps == 1 and int(tr.step_dev.item()) == 1
        g = _f64(m.flat.G) / n_acc
        n64 = float(np.sqrt((g * g).sum()))
        coef64 = float(np.float32(0.02)) / (n64 + 1e-6)
        print("N = %d: norm %.6g coef %.6g" % (n_acc, n64, coef64))
        assert coef64 < 1.0
        assert _within_one_ulp(tr.last_grad_norm.item(), np.float32(n64))
        assert abs(float(tr._clip_stat[1].item()) - coef64) < 1e-6 * max(1.0, coef64)
        p64, _, _ = _adamw64(p0, g * coef64, 0.0, 0.0, lr=1e-3, step=1)
        # (a first step's P is nearly scale-free: the coefficient is pinned by _clip_stat[1] above and by the moments below)
        assert np.abs(_f64(m.flat.P) - p64).max() < 1e-6
        _check_moments(m.flat, g * coef64)


# ---- 6. two ranks --------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q, batch, clip):
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
        tr = Trainer(m, lr=1e-3, graph=False, gradient_clip_val=clip)
        tr.train_step(batch[0].to(dev), batch[1].to(dev))
        torch.cuda.synchronize()
        q.put((rank, tr._clip_stat.cpu().numpy(), m.flat.P.cpu().numpy(), m.flat.M.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_by_the_same_norm_and_equal_one_process(dev):
    """Two ranks on one GPU, one micro-batch each: after the exchange both hold the same G and reduce it in the same order,
    so norm, coefficient and parameters are bit-equal across ranks with no extra collective; the step equals ONE process
    accumulating both micro-batches (N = 2, the same 1/2 scale) to the tolerance of the unclipped two-rank test."""
    from mrmt3.synthetic import synth_mel, synth_labels
    from mrmt3.trainer import Trainer
    micro = [(torch.from_numpy(synth_mel(2, seed=200 + i)), torch.from_numpy(synth_labels(2, 128, seed=300 + i)))
             for i in range(2)]

    def one_process(**kw):
        m = _model("t5", torch.bfloat16, dev, dropout_rate=0.0)
        start = m.flat.P.detach().cpu().numpy().copy()
        tr = Trainer(m, lr=1e-3, graph=False, accumulate_grad_batches=2, **kw)
        for mel, lab in micro:
            tr.train_step(mel.to(dev), lab.to(dev))
        torch.cuda.synchronize()
        return start, m.flat.P.cpu().numpy(), m.flat.M.cpu().numpy(), tr._clip_stat.cpu().numpy()

    _, _, _, stat = one_process(track_grad_norm=True)
    clip = float(stat[0]) / 2
    assert np.isfinite(clip) and clip > 0
    start, p1, m1, stat1 = one_process(gradient_clip_val=clip)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, micro[r], clip)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, s0, pa, ma), (_, s1, pb, mb) = res
    assert s0.tobytes() == s1.tobytes()                       # norm, coef, skip: the same bits on both ranks
    assert np.array_equal(pa, pb) and np.array_equal(ma, mb)
    assert 0.4 < s0[1] < 0.6 and s0[2] == 0
    assert abs(float(s0[0]) - float(stat1[0])) / float(stat1[0]) < 1e-5      # (the gradients agree to 1e-5, test_grad_accum_gpu)
    du, dw = pa - start, p1 - start
    assert np.linalg.norm(du - dw) / np.linalg.norm(dw) < 1e-3
    assert np.linalg.norm(ma - m1) / np.linalg.norm(m1) < 1e-3


# ---- 7. the non-finite guard ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan")])
def test_abi_nonfinite_gradient_skips_the_step(dev, poison):
    from mrmt3 import lib
    n = 4 * 50000
    gen = torch.Generator(device=dev).manual_seed(2)
    p, g, m, v = (torch.randn(n, device=dev, generator=gen) for _ in range(4))
    v = v.abs()
    g[12345] = poison
    s = torch.randn(n, device=dev, generator=gen).bfloat16()
    skipped = torch.zeros(1, device=dev, dtype=torch.int32)
    ws, stat = lib.grad_norm_workspace(dev), torch.zeros(4, device=dev)
    lr = torch.full((1,), 1e-3, device=dev)
    step = torch.full((1,), 3, device=dev, dtype=torch.int32)
    lib.grad_norm(g, 0.5, 1.0, True, ws, stat, skipped)
    P, M, V, S = p.clone(), m.clone(), v.clone(), s.clone()
    lib.adamw_step(P, g, M, V, lr, step, grad_scale=0.5, stat=stat, shadow=S)
    torch.cuda.synchronize()
    st = stat.cpu().numpy()
    assert not np.isfinite(st[0]) and st[1] == 0.0 and st[2] == 1.0 and int(skipped.item()) == 1
    for x, y in ((P, p), (M, m), (V, v), (S.view(torch.int16), s.view(torch.int16))):
        assert torch.equal(x, y)
    assert int(step.item()) == 4                              # an ATTEMPTED step: the counter advances
    # a second bad step counts on; a finite gradient clears the flag and updates
    lib.grad_norm(g, 0.5, 1.0, True, ws, stat, skipped)
    g[12345] = 0.0
    torch.cuda.synchronize()
    assert int(skipped.item()) == 2
    lib.grad_norm(g, 0.5, 1.0, True, ws, stat, skipped)
    lib.adamw_step(P, g, M, V, lr, step, grad_scale=0.5, stat=stat, shadow=S)
    torch.cuda.synchronize()
    st = stat.cpu().numpy()
    assert np.isfinite(st[0]) and 0 < st[1] < 1 and st[2] == 0.0 and int(skipped.item()) == 2 and int(step.item()) == 5
    assert not torch.equal(P, p) and bool(torch.isfinite(P).all())
    # without the guard the flag stays down and the norm says what happened
    g[12345] = poison
    st, k = _run_norm(g, 0.5, max_norm=1.0, skip=False)
    assert not np.isfinite(st[0]) and st[2] == 0.0 and k == 0


def _poison(m, value):
    w = m.flat.master("lm_head.weight")
    old = float(w[3, 5].item())
    w[3, 5] = value
    return old


def test_trainer_skips_a_nonfinite_step_under_graph_replay_and_recovers(dev):
    """bf16, dropout on, skip_nonfinite: after the capture one lm_head master weight is set to +inf (the shadows follow), the
    replayed step sees a non-finite norm and changes nothing — P, M, V keep every bit, skipped_steps = 1, step_dev and
    host_step advance together; with the weight restored the next replay updates again and the whole run equals its eager
    twin bit for bit."""
    from mrmt3.trainer import Trainer
    data = [_micro(dev, B=2, L=128, seed=80 + i) for i in range(5)]
    runs = {}
    for use_graph in (True, False):
        m = _model("t5", torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=use_graph, skip_nonfinite=True)
        for x in data[:3]:
            tr.train_step(*x)
        torch.cuda.synchronize()
        assert tr.graph_captured == use_graph and tr.skipped_steps == 0
        assert float(tr._clip_stat[1].item()) == 1.0 and np.isfinite(float(tr.last_grad_norm.item()))
        old = _poison(m, float("inf"))
        before = [t.clone() for t in (m.flat.P, m.flat.M, m.flat.V)]
        tr.train_step(*data[3])
        torch.cuda.synchronize()
        assert tr.skipped_steps == 1 and not np.isfinite(float(tr.last_grad_norm.item()))
        for x, y in zip(before, (m.flat.P, m.flat.M, m.flat.V)):
            assert torch.equal(x, y)
        assert tr.optimizer_steps == 4 and int(tr.step_dev.item()) == 4
        _poison(m, old)
        assert bool(torch.isfinite(m.flat.P).all())
        tr.train_step(*data[4])
        torch.cuda.synchronize()
        assert tr.skipped_steps == 1 and np.isfinite(float(tr.last_grad_norm.item())) and int(tr.step_dev.item()) == 5
        assert not torch.equal(before[0], m.flat.P) and bool(torch.isfinite(m.flat.P).all())
        assert bool(torch.isfinite(m.flat.M).all()) and bool(torch.isfinite(m.flat.V).all())
        runs[use_graph] = [t.clone() for t in (m.flat.P, m.flat.M, m.flat.V)]
        tr.close()
    for x, y in zip(runs[True], runs[False]):
        assert torch.equal(x, y)


def test_without_the_guard_a_nonfinite_gradient_propagates_like_torch(dev):
    from mrmt3.trainer import Trainer
    m = _model("t5", torch.bfloat16, dev, dropout_rate=0.0)
    tr = Trainer(m, lr=1e-3, graph=False, gradient_clip_val=1.0)
    _poison(m, float("inf"))
    tr.train_step(*_micro(dev, B=2, L=128, seed=90))
    torch.cuda.synchronize()
    assert tr.skipped_steps == 0 and int(tr.step_dev.item()) == 1
    assert not np.isfinite(float(tr.last_grad_norm.item()))


# ---- 8. train.py ---------------------------------------------------------------------------------------------------
TOP = """
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


def test_train_py_logs_the_gradient_norm_only_when_clipping_is_on(dev, tmp_path, monkeypatch, capsys):
    import train
    from mrmt3 import trainer as trainer_mod
    from test_config_cpu import MODEL
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
    base = ["--config-dir", str(tmp_path / "cfg"), "--config-name", "config", "+synthetic=True", f"+output_dir={tmp_path / 'out'}"]
    train.main(base + ["+max_steps=4", "+trainer.gradient_clip_val=0.05", "+skip_nonfinite=true"])
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("step ")]
    assert len(lines) == 4 and all(re.fullmatch(r"step \d+ train_loss \d+\.\d{4} grad_norm \d+\.\d{4}", x) for x in lines), lines
    tr = made[-1]
    assert tr.clip_on and tr._max_norm == 0.05 and tr._clip_value == 0.0 and tr.skip_nonfinite and tr.skipped_steps == 0
    assert all(float(x.split()[-1]) > 0 for x in lines)
    train.main(base + ["+max_steps=2", "+trainer.gradient_clip_val=0.5", "+trainer.gradient_clip_algorithm=value"])
    capsys.readouterr()
    assert made[-1]._clip_value == 0.5 and made[-1]._max_norm == 0.0
    train.main(base + ["+max_steps=2"])
    out = capsys.readouterr().out
    lines = [x for x in out.splitlines() if x.startswith("step ")]
    assert len(lines) == 2 and all(re.fullmatch(r"step \d+ train_loss \d+\.\d{4}", x) for x in lines), lines
    assert "grad_norm" not in out and "skipped_steps" not in out and not made[-1].clip_on
