"""Label smoothing and z-loss in the fused cross-entropy (mrmt3_ce_fwd_bwd_reg, mrmt3_lmhead_ce_fwd_bwd_reg,
`Trainer(label_smoothing=, z_loss=)`) on the MI355X.  The reference is always the float64 closed form of
tests/loss_ref.py on the CPU (pinned to torch and to autograd by tests/test_loss_options_cpu.py), never a kernel."""
import functools

import numpy as np
import pytest
import torch

import loss_ref
from test_grad_accum_gpu import _micro, _model, _rel

pytestmark = pytest.mark.gpu

OPTIONS = [(0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=4)
def _case(rows, V, weighted):
    logits, targets = loss_ref.case(rows, V, weighted)
    return logits, targets, logits.cuda(), targets.cuda()


@functools.lru_cache(maxsize=4)
def _reference(rows, V, weighted, eps, z):
    logits, targets, _, _ = _case(rows, V, weighted)
    lo, hi = loss_ref.inst_range(V)
    obj, nll = loss_ref.objective(logits, targets, eps, z, weighted, lo, hi)
    return float(obj), float(nll), loss_ref.gradient(logits, targets, eps, z, weighted, lo, hi)


GUARD = 3          # rows behind the gradient's last row that the kernel must leave alone


def _abi_reg(logits, targets, eps, z, weighted, lo, hi, dtype=torch.float32, grad_scale=1.0):
    """mrmt3_ce_count + mrmt3_ce_fwd_bwd_reg through the C ABI -> (objective, nll) as float64, dlogits [rows, V] and the
    guard rows behind it (filled with 7 before the launch)."""
    from mrmt3 import lib
    rows, V = logits.shape
    so = lib.load()
    acc = torch.zeros(3, device=logits.device, dtype=torch.float64)           # objective, nll, denom (f32 in its first 4 bytes)
    den = lib.C.c_void_p(acc.data_ptr() + 16)
    buf = torch.full((rows + GUARD, V), 7.0, device=logits.device, dtype=dtype)
    lib._check(so.mrmt3_ce_count(lib._p(targets), rows, int(weighted), lo, hi, den, lib._stream()), "ce_count")
    lib._check(so.mrmt3_ce_fwd_bwd_reg(lib._p(logits), lib._p(targets), den, eps, z, lib._p(acc), lib._p(buf), lib._dt(buf),
                                       rows, V, int(weighted), lo, hi, grad_scale, lib._stream()), "ce_fwd_bwd_reg")
    torch.cuda.synchronize()
    return float(acc[0].item()), float(acc[1].item()), buf[:rows], buf[rows:]


# ---- 1. the kernels, f32 gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps,z", OPTIONS)
@pytest.mark.parametrize("rows", [37, 8200])
@pytest.mark.parametrize("V", [1536, 512, 2048, 1100])
def test_reg_kernels_equal_the_float64_closed_form(dev, V, rows, eps, z, weighted):
    """Wave kernel (V = 1536, 512, 2048) and general kernel (V = 1100: a multiple of 4, not of 256); 37 rows = a ragged last
    workgroup, 8200 rows = one row per wave with a ragged tail.  Tolerances of test_cross_entropy: both scalars within
    1e-5 * max(1, |ref|), the gradient atol 1e-8 / rtol 1e-4; ignored rows exactly zero; guard rows untouched.  With
    `weighted` every odd row's target lies in the instrument range (1135..1262 where the vocabulary holds it, else a range
    of the same width passed as inst_lo / inst_hi: a target must stay below V)."""
    _, targets, lg, tg = _case(rows, V, weighted)
    lo, hi = loss_ref.inst_range(V)
    obj_ref, nll_ref, g_ref = _reference(rows, V, weighted, eps, z)
    obj, nll, g, guard = _abi_reg(lg, tg, eps, z, weighted, lo, hi)
    g = g.double().cpu()
    err = float((g - g_ref).abs().max())
    print("V %d rows %d eps %g z %g weighted %d: objective %.9g (ref %.9g, d %.2e) nll %.9g (ref %.9g, d %.2e) max|dg| %.2e"
          % (V, rows, eps, z, weighted, obj, obj_ref, abs(obj - obj_ref), nll, nll_ref, abs(nll - nll_ref), err))
    assert abs(obj - obj_ref) < 1e-5 * max(1.0, abs(obj_ref))
    assert abs(nll - nll_ref) < 1e-5 * max(1.0, abs(nll_ref))
    assert torch.allclose(g, g_ref, atol=1e-8, rtol=1e-4)
    assert float(g[targets == -100].abs().max()) == 0.0
    assert bool((guard == 7.0).all())


# ---- 2. bf16 gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps,z", OPTIONS)
def test_reg_wave_kernel_bf16_gradient_is_the_f32_value_rounded_once(dev, eps, z, weighted):
    """V = 1536, 37 rows, bf16 dlogits: every element within 2^-8 |ref| + 1e-8 of the float64 gradient (half a bf16 ulp is
    2^-9 relative, doubled for the f32 error in front of the rounding)."""
    rows, V = 37, 1536
    _, targets, lg, tg = _case(rows, V, weighted)
    lo, hi = loss_ref.inst_range(V)
    obj_ref, nll_ref, g_ref = _reference(rows, V, weighted, eps, z)
    obj, nll, g, guard = _abi_reg(lg, tg, eps, z, weighted, lo, hi, dtype=torch.bfloat16)
    g = g.double().cpu()
    excess = (g - g_ref).abs() - (2.0 ** -8 * g_ref.abs() + 1e-8)
    print("bf16 eps %g z %g weighted %d: worst |d| / (2^-8 |ref| + 1e-8) = %.3f"
          % (eps, z, weighted, float(((g - g_ref).abs() / (2.0 ** -8 * g_ref.abs() + 1e-8)).max())))
    assert float(excess.max()) <= 0.0
    assert abs(obj - obj_ref) < 1e-5 * max(1.0, abs(obj_ref)) and abs(nll - nll_ref) < 1e-5 * max(1.0, abs(nll_ref))
    assert float(g[targets == -100].abs().max()) == 0.0 and bool((guard == 7.0).all())


# ---- 3. off means unchanged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1536, 1100])
def test_options_off_is_the_old_entry_point_bit_for_bit(dev, V, monkeypatch):
    from mrmt3 import lib
    rows = 37
    _, targets, lg, tg = _case(rows, V, True)
    lo, hi = loss_ref.inst_range(V)
    loss0, dl0 = lib.cross_entropy(lg, tg, grad_dtype=torch.float32, weighted=True, inst_lo=lo, inst_hi=hi)
    so = lib.load()

    def boom(*a):
        raise AssertionError("both options are off: the new entry point may not be called")
    monkeypatch.setattr(so, "mrmt3_ce_fwd_bwd_reg", boom)
    loss1, dl1 = lib.cross_entropy(lg, tg, grad_dtype=torch.float32, weighted=True, inst_lo=lo, inst_hi=hi,
                                   label_smoothing=0, z_loss=0)
    loss2, dl2, nll2 = lib.cross_entropy(lg, tg, grad_dtype=torch.float32, weighted=True, inst_lo=lo, inst_hi=hi,
                                         label_smoothing=0.0, z_loss=0.0, return_nll=True)
    assert torch.equal(loss0, loss1) and torch.equal(dl0, dl1) and torch.equal(loss0, loss2) and torch.equal(dl0, dl2)
    assert nll2 is loss2
    monkeypatch.undo()
    # the REG kernels with (0, 0): objective == nll exactly, gradient within the f32 tolerance of the old path's
    obj, nll, g, guard = _abi_reg(lg, tg, 0.0, 0.0, True, lo, hi)
    assert obj == nll
    assert abs(obj - float(loss0.item())) < 1e-5 * max(1.0, abs(obj))
    assert torch.allclose(g, dl0, atol=1e-8, rtol=1e-4)
    assert bool((guard == 7.0).all())
    # and the wrapper with an option on: (objective, dlogits), the NLL on request
    obj_ref, nll_ref, g_ref = _reference(rows, V, True, 0.1, 1e-4)
    two = lib.cross_entropy(lg, tg, grad_dtype=torch.float32, weighted=True, inst_lo=lo, inst_hi=hi, label_smoothing=0.1,
                            z_loss=1e-4)
    assert len(two) == 2 and two[0].shape == (1,) and two[0].dtype == torch.float32
    o3, dl3, n3 = lib.cross_entropy(lg, tg, grad_dtype=torch.float32, weighted=True, inst_lo=lo, inst_hi=hi,
                                    label_smoothing=0.1, z_loss=1e-4, return_nll=True)
    assert torch.equal(two[1], dl3) and torch.equal(two[0], o3)
    assert abs(float(o3.item()) - obj_ref) < 1e-5 * max(1.0, abs(obj_ref))
    assert abs(float(n3.item()) - nll_ref) < 1e-5 * max(1.0, abs(nll_ref))
    assert torch.allclose(dl3.double().cpu(), g_ref, atol=1e-8, rtol=1e-4)
    o4, none, n4 = lib.cross_entropy(lg, tg, want_grad=False, weighted=True, inst_lo=lo, inst_hi=hi, label_smoothing=0.1,
                                     z_loss=1e-4, return_nll=True)
    assert none is None and abs(float(o4.item()) - obj_ref) < 1e-5 * max(1.0, abs(obj_ref))
    assert abs(float(n4.item()) - nll_ref) < 1e-5 * max(1.0, abs(nll_ref))


# ---- 4. the chunked lm_head form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32])
def test_lmhead_ce_reg_chunks_equal_gemm_then_ce_reg(dev, grad_dtype):
    """300 rows in chunks of 128 (three chunks, the last ragged) == mrmt3_gemm_nt, then mrmt3_ce_fwd_bwd_reg on the whole
    tensor: the gradient bit for bit, the two scalars to 1e-12 relative (double accumulators: order-dependent at 1e-16)."""
    from mrmt3 import lib
    rows, d, V, chunk = 300, 512, 1536, 128
    gen = torch.Generator(device=dev).manual_seed(7)
    dec = torch.randn(rows, d, device=dev, generator=gen).bfloat16()
    w = (torch.randn(V, d, device=dev, generator=gen) * 0.05).bfloat16()
    tg = loss_ref.case(rows, V, True, seed=3)[1].to(dev)
    eps, z = 0.1, 1e-4
    so = lib.load()

    def run(chunked):
        acc = torch.zeros(3, device=dev, dtype=torch.float64)
        den = lib.C.c_void_p(acc.data_ptr() + 16)
        dl = torch.full((rows + GUARD, V), 7.0, device=dev, dtype=grad_dtype)
        lib._check(so.mrmt3_ce_count(lib._p(tg), rows, 1, 1135, 1262, den, lib._stream()), "ce_count")
        if chunked:
            ws = torch.empty(chunk * V, device=dev, dtype=torch.float32)
            lib._check(so.mrmt3_lmhead_ce_fwd_bwd_reg(lib._p(dec), dec.stride(0), lib._p(w), w.stride(0), lib._p(tg), den, eps, z,
                                                      lib._p(acc), lib._p(dl), lib._dt(dl), rows, V, d, 1, 1135, 1262, 1.0,
                                                      lib._p(ws), ws.numel() * 4, chunk, lib._stream()), "lmhead_ce_fwd_bwd_reg")
        else:
            logits = lib.gemm_nt(dec, w, out_dtype=torch.float32)
            lib._check(so.mrmt3_ce_fwd_bwd_reg(lib._p(logits), lib._p(tg), den, eps, z, lib._p(acc), lib._p(dl), lib._dt(dl),
                                               rows, V, 1, 1135, 1262, 1.0, lib._stream()), "ce_fwd_bwd_reg")
        torch.cuda.synchronize()
        assert bool((dl[rows:] == 7.0).all())
        return acc[:2].cpu().numpy(), dl[:rows].clone()

    (sa, ga), (sb, gb) = run(False), run(True)
    print("chunked vs whole: scalars", sa, sb)
    assert torch.equal(ga, gb)
    assert np.all(np.abs(sa - sb) <= 1e-12 * np.abs(sa)) and sa[0] != sa[1] and np.all(sa > 0)
    # the wrapper takes the same road
    o, dl, n = lib.lmhead_cross_entropy(dec, w, tg, grad_dtype=grad_dtype, weighted=True, chunk_rows=chunk, label_smoothing=eps,
                                        z_loss=z, return_nll=True)
    assert torch.equal(dl, ga)
    assert abs(float(o.item()) - sb[0]) <= 1e-6 * sb[0] and abs(float(n.item()) - sb[1]) <= 1e-6 * sb[1]     # (returned as f32)
    # against float64 on the f32 logits the GEMM produced
    logits = lib.gemm_nt(dec, w, out_dtype=torch.float32).cpu()
    obj_ref, nll_ref = loss_ref.objective(logits, tg.cpu(), eps, z, True)
    assert abs(sb[0] - float(obj_ref)) < 1e-5 * max(1.0, abs(float(obj_ref)))
    assert abs(sb[1] - float(nll_ref)) < 1e-5 * max(1.0, abs(float(nll_ref)))


# ---- 5. the trainer, fp32 engine -------------------------------------------------------------------------------------
def _equal_length_batch(dev):
    """The fixture of tests/test_grad_clip_gpu.py (B = 2, short Slakh-shaped labels, -100 padding), both rows cut to the
    shorter row's length: with equal token counts the mean of the two half-batch means is the batch mean, which is what the
    accumulation check below needs (test_two_half_micro_batches_equal_one_full_batch uses full-length labels for that)."""
    mel, lab = _micro(dev, B=2, L=192, seed=40, mean_len=60)
    n = int((lab != -100).sum(1).min().item())
    assert 2 <= n < 128
    lab[:, n - 1] = 1
    lab[:, n:] = -100
    return mel, lab


def _trainer_grads(dev, batch, micro=None, **kw):
    from mrmt3.trainer import Trainer
    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    tr = Trainer(m, lr=1e-3, graph=False, label_smoothing=0.1, z_loss=1e-4, **kw)
    seen = []
    for mel, lab in (micro or [batch]):
        tr.train_step(mel, lab)
        seen.append((float(tr.last_loss.item()), float(tr.last_nll.item())))
    torch.cuda.synchronize()
    assert tr.optimizer_steps == 1
    n = tr.accumulate
    return seen, {k: m.flat.grad(k).detach().double().cpu() / n for k in m.flat.shapes}, tr


def test_fp32_trainer_step_with_options_equals_oracle_autograd(dev):
    """One train_step with (0.1, 1e-4), dense: every gradient tensor within rel-L2 1e-4 of the oracle's float64 autograd of
    the closed-form objective on oracle.t5_ref logits (the bound test_fp32_gradients_match_oracle asserts in
    tests/test_model_gpu.py); last_loss is the objective and last_nll the plain CE within 1e-5 * max(1, |ref|).  Packed: the
    same objective to 1e-6 and gradients within rel-L2 2e-6 of the dense step (test_packed_fp32_engine_equals_dense_and_oracle).
    Two half-batches accumulated: the one-batch gradient within rel-L2 2e-6 (test_two_half_micro_batches_equal_one_full_batch)."""
    from mrmt3.synthetic import T5_SMALL, golden_weights
    from oracle import t5_ref
    mel, lab = _equal_length_batch(dev)
    (dense,), gd, tr = _trainer_grads(dev, (mel, lab))
    assert tr.loss_reg and tr.pack_capacity(lab) is None
    torch.set_num_threads(8)
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in golden_weights(T5_SMALL, 0).items()}
    logits = t5_ref.forward_logits(sd, T5_SMALL, mel.cpu().double(), lab.cpu())
    obj, nll = loss_ref.objective(logits.reshape(-1, logits.shape[-1]), lab.cpu().reshape(-1), 0.1, 1e-4)
    obj.backward()
    obj, nll = float(obj.detach()), float(nll.detach())
    print("trainer: objective %.7f (oracle %.7f) nll %.7f (oracle %.7f)" % (dense[0], obj, dense[1], nll))
    assert abs(nll - float(t5_ref.ce_loss(logits, lab.cpu()).detach())) < 1e-12
    assert abs(dense[0] - obj) < 1e-5 * max(1.0, abs(obj)) and abs(dense[1] - nll) < 1e-5 * max(1.0, abs(nll))
    assert abs(obj - nll) > 1e-3                       # the two scalars are different numbers
    worst = 0.0
    for k, v in sd.items():
        if v.grad is None or v.grad.norm() == 0:
            assert gd[k].norm() < 1e-7, k
            continue
        worst = max(worst, _rel(gd[k], v.grad))
        assert _rel(gd[k], v.grad) < 1e-4, (k, _rel(gd[k], v.grad))
    print("trainer: worst rel-L2 against the float64 oracle %.2e" % worst)

    (packed,), gp, trp = _trainer_grads(dev, (mel, lab), pack_targets=True)
    assert trp.pack_capacity(lab) is not None
    assert abs(packed[0] - dense[0]) <= 1e-6 and abs(packed[1] - dense[1]) <= 1e-6, (packed, dense)
    halves, ga, _ = _trainer_grads(dev, None, micro=[(mel[0:1], lab[0:1]), (mel[1:2], lab[1:2])], accumulate_grad_batches=2)
    # equal token counts: the batch scalars are the means of the micro-batch scalars (1e-6: two f32 roundings of values < 10)
    assert abs((halves[0][0] + halves[1][0]) / 2 - dense[0]) < 2e-6 and abs((halves[0][1] + halves[1][1]) / 2 - dense[1]) < 2e-6
    for k, g in gd.items():
        if g.norm() == 0:
            assert gp[k].norm() < 1e-7 and ga[k].norm() < 1e-7, k
            continue
        assert _rel(gp[k], g) <= 2e-6, ("packed", k, _rel(gp[k], g))
        assert _rel(ga[k], g) <= 2e-6, ("accumulated", k, _rel(ga[k], g))


def test_fp32_trainer_weighted_clipped_step_with_options(dev):
    """weighted_loss and clipping with the options on: the objective follows the weighted closed form on the engine's own
    logits, and the clipped tail still runs (a finite norm, a coefficient below 1)."""
    from mrmt3.trainer import Trainer
    mel, lab = _equal_length_batch(dev)
    lab = lab.clone()
    lab[:, 3:9] = 1200                                   # instrument tokens: weight 3, count 2
    m = _model("t5", torch.float32, dev, dropout_rate=0.0)
    with torch.no_grad():
        logits = m(inputs=mel, labels=lab).float().cpu()
    obj, nll = loss_ref.objective(logits.reshape(-1, logits.shape[-1]), lab.cpu().reshape(-1), 0.1, 1e-4, weighted=True)
    tr = Trainer(m, lr=1e-3, graph=False, weighted_loss=True, gradient_clip_val=1e-3, label_smoothing=0.1, z_loss=1e-4)
    loss = tr.train_step(mel, lab)
    torch.cuda.synchronize()
    assert loss is tr.last_loss
    assert abs(float(loss.item()) - float(obj)) < 1e-5 * max(1.0, abs(float(obj)))
    assert abs(float(tr.last_nll.item()) - float(nll)) < 1e-5 * max(1.0, abs(float(nll)))
    assert np.isfinite(float(tr.last_grad_norm.item())) and 0.0 < float(tr._clip_stat[1].item()) < 1.0


# ---- 6. the trainer, bf16 engine, graph ------------------------------------------------------------------------------
def _spy(monkeypatch, so, names):
    calls = {n: 0 for n in names}
    for n in names:
        fn = getattr(so, n)

        def wrapper(*a, _fn=fn, _n=n):
            calls[_n] += 1
            return _fn(*a)
        monkeypatch.setattr(so, n, wrapper)
    return calls


CE_ENTRIES = ("mrmt3_ce_fwd_bwd", "mrmt3_lmhead_ce_fwd_bwd", "mrmt3_ce_fwd_bwd_reg", "mrmt3_lmhead_ce_fwd_bwd_reg")


def test_bf16_graph_replay_with_options_and_untouched_step_when_off(dev, monkeypatch):
    """bf16, dropout on, (0.1, 1e-4): two eager warm-ups and one replay; the replayed step's objective, NLL and weights are
    bit-equal to the eager trainer's.  A trainer with both options off issues the same dispatch counts for one step, calls
    the old lm_head + CE entry point once and the new ones never; last_nll is last_loss there."""
    from mrmt3 import lib
    from mrmt3.trainer import Trainer
    data = [_micro(dev, B=2, L=192, seed=40 + i, mean_len=60) for i in range(3)]
    runs = {}
    for use_graph in (False, True):
        m = _model("t5", torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=use_graph, label_smoothing=0.1, z_loss=1e-4)
        seen = []
        for x in data:
            loss = tr.train_step(*x)
            seen.append((float(loss.item()), float(tr.last_nll.item())))
        torch.cuda.synchronize()
        assert tr.graph_captured == use_graph
        if use_graph:
            assert all(len(s) == 5 for s in tr._graphs), list(tr._graphs)       # the options are part of no signature
        runs[use_graph] = (seen, m.flat.P.clone(), m.flat.M.clone())
        tr.close()
    print("eager", runs[False][0], "graph", runs[True][0])
    assert runs[False][0] == runs[True][0]
    assert torch.equal(runs[False][1], runs[True][1]) and torch.equal(runs[False][2], runs[True][2])
    assert all(np.isfinite(o) and np.isfinite(n) and o != n for o, n in runs[True][0])

    so = lib.load()
    counts = {}
    for on in (False, True):
        m = _model("t5", torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=False, **({"label_smoothing": 0.1, "z_loss": 1e-4} if on else {}))
        tr.train_step(*data[0])                          # (tables and workspaces of the first step)
        torch.cuda.synchronize()
        calls = _spy(monkeypatch, so, CE_ENTRIES)
        lib.dispatch_counts(reset=True)
        tr.train_step(*data[1])
        torch.cuda.synchronize()
        counts[on] = lib.dispatch_counts()
        monkeypatch.undo()
        want = {n: 0 for n in CE_ENTRIES}
        want["mrmt3_lmhead_ce_fwd_bwd_reg" if on else "mrmt3_lmhead_ce_fwd_bwd"] = 1
        assert calls == want, (on, calls)
        assert tr.loss_reg == on and (tr.last_nll is tr.last_loss) == (not on)
        tr.close()
    assert counts[False] == counts[True] and counts[False]["gemm_nt8"] + counts[False]["gemm_nt_tile"] > 0, counts


# ---- 7. evaluation stays the plain NLL -------------------------------------------------------------------------------
def test_eval_loss_and_score_ignore_the_options(dev, monkeypatch):
    """A model whose trainer has the options on: eval_loss is bit-equal to that of a trainer without them, score is what it
    was before the trainer existed, and neither goes near the new entry points."""
    from mrmt3 import lib
    from mrmt3.trainer import Trainer
    mel, lab = _micro(dev, B=2, L=192, seed=40, mean_len=60)
    m = _model("t5", torch.bfloat16, dev)
    s_off = m.score(mel, lab)
    off = Trainer(m, lr=1e-3, graph=False)
    e_off = off.eval_loss(mel, lab)
    on = Trainer(m, lr=1e-3, graph=False, label_smoothing=0.1, z_loss=1e-4)
    calls = _spy(monkeypatch, lib.load(), CE_ENTRIES)
    e_on = on.eval_loss(mel, lab)
    s_on = m.score(mel, lab)
    torch.cuda.synchronize()
    assert calls == {"mrmt3_ce_fwd_bwd": 0, "mrmt3_lmhead_ce_fwd_bwd": 1, "mrmt3_ce_fwd_bwd_reg": 0, "mrmt3_lmhead_ce_fwd_bwd_reg": 0}
    assert torch.equal(e_on, e_off) and torch.equal(s_on, s_off)
    assert float(e_on.item()) > 0 and bool((s_on[lab == -100] == 0).all())
    on.close()
    off.close()
