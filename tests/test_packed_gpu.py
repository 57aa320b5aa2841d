"""Packed decoder training on the MI355X: the pack kernel, the varlen attention kernels against the dense ones per row prefix,
the packed engine against the dense engine and the oracle, and the trainer's packed step (eager, captured, several Tcap)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
H = 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _labels_with(lengths, L, seed=0):
    rs = np.random.RandomState(seed)
    lab = rs.randint(3, 1391, size=(len(lengths), L)).astype(np.int64)
    for b, n in enumerate(lengths):
        lab[b, n:] = -100
    return torch.from_numpy(lab)


def _plan(lab, dev):
    from mrmt3 import lib, packing
    B, L = lab.shape
    tcap = packing.capacity(packing.row_lengths(lab.numpy()), B, L)
    return lib.pack_plan(lab.to(dev).contiguous(), tcap, 0, 0)


@pytest.mark.parametrize("lengths,L", [([0, 1024, 37], 1024), ([1024], 1024), ([5], 1024), ([256, 0], 256),
                                       ([200, 56, 0, 1], 256)])
def test_pack_plan_matches_restatement(dev, lengths, L):
    """row_off, tok_row, tok_pos, dec_ids, targets against a torch restatement: an empty row, a full row, B = 1, T exactly on a
    granule (256 + 0 with a 256 granule), and an error case (T > Tcap: clamped, flagged, nothing written past Tcap)."""
    from mrmt3 import lib, packing
    lab = _labels_with(lengths, L)
    B = len(lengths)
    if sum(lengths) == 257:                         # T = 257 > Tcap = 256 on purpose: the error word
        pl = lib.pack_plan(lab.to(dev), 256, 0, 0)
        torch.cuda.synchronize()
        assert int(pl.err.item()) == 1 and int(pl.row_off[-1].item()) == 256
        return
    tcap = packing.capacity(packing.row_lengths(lab.numpy()), B, L)
    pl = lib.pack_plan(lab.to(dev), tcap, 0, 0)
    torch.cuda.synchronize()
    assert int(pl.err.item()) == 0
    off = np.concatenate([[0], np.cumsum(lengths)])
    assert pl.len.cpu().tolist() == list(lengths)
    assert pl.row_off.cpu().tolist() == off.tolist()
    T = off[-1]
    rows, pos, ids, tg = [], [], [], []
    for b, n in enumerate(lengths):
        for t in range(n):
            rows.append(b)
            pos.append(t)
            prev = 0 if t == 0 else int(lab[b, t - 1])
            ids.append(0 if prev == -100 else prev)
            tg.append(int(lab[b, t]))
    tail = tcap - T
    assert pl.tok_row.cpu().tolist() == rows + [-1] * tail
    assert pl.tok_pos.cpu().tolist() == pos + [0] * tail
    assert pl.dec_ids.cpu().tolist() == ids + [0] * tail
    assert pl.targets.cpu().tolist() == tg + [-100] * tail
    tiles = pl.tiles.cpu().numpy()
    used = int(tiles[0])
    ent = tiles[2:].reshape(-1, 2)
    assert used == sum((n + 63) // 64 for n in lengths) and int(tiles[1]) == T
    assert sorted(map(tuple, ent[:used].tolist())) == sorted((b, t) for b, n in enumerate(lengths) for t in range((n + 63) // 64))
    assert list(ent[:used, 1]) == sorted(ent[:used, 1], reverse=True)       # heaviest causal tile first
    assert (ent[used:, 0] == -1).all() and len(ent) - used >= -(-tail // 64)


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _varlen_fwd_raw(q, k, v, pl, Lk, causal, p, lib):
    """mrmt3_attn_fwd_varlen into NaN-filled outputs (the tail must come back as zeros)."""
    T = pl.Tcap
    o = _nan((T, H * 64), q.dtype, q.device)
    lo = _nan((T, H * 64), q.dtype, q.device) if q.dtype == torch.bfloat16 else None
    lse = _nan((H, T), torch.float32, q.device)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib._check(lib.load().mrmt3_attn_fwd_varlen(vp(q), q.stride(0), vp(k), k.stride(0), vp(v), v.stride(0), vp(o), o.stride(0),
                                                vp(lo), vp(lse), vp(pl.row_off), vp(pl.tiles), pl.B, H, T, pl.L, Lk, int(causal),
                                                lib._dt(q), p, 7, None, 3, lib._stream()), "attn_fwd_varlen")
    return o, lse, lo


def _close_ulp(a, b, ulps):
    a, b = a.float(), b.float()
    if ulps == 0:
        return torch.equal(a, b)
    tol = torch.maximum(a.abs(), b.abs()) * (2.0 ** -7) * ulps + 1e-30
    return bool(((a - b).abs() <= tol).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("site", ["self", "cross256", "cross320"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_varlen_attention_equals_dense_per_row_prefix(dev, knobs, dtype, site, p):
    """Forward o / lse and dQ / dK / dV of the varlen kernels against the dense kernels (two-pass backward,
    MRMT3_ATTN_ONEPASS=0) on each row's prefix, dO zeroed past each row's length.  f32: bit for bit.  bf16: bit for bit is
    expected (the key tiles start at the same in-row offsets and are summed in the same order; the extra all-zero query rows of
    the dense dK/dV add exact zeros); at most 1 bf16 ulp is accepted in case the MFMA accumulation order of such zero terms
    ever differs.  Tail rows of every output (NaN-filled beforehand) come back exactly 0."""
    from mrmt3 import lib
    knobs.set("MRMT3_ATTN_ONEPASS", 0)
    L, lengths = 256, [100, 256]
    B = len(lengths)
    causal = site == "self"
    Lk = {"self": 0, "cross256": 256, "cross320": 320}[site]
    Lkd = L if causal else Lk
    g = torch.Generator(device="cpu").manual_seed(1)
    mk = lambda r: (torch.randn(r, H * 64, generator=g) * 0.5).to(dev, dtype)
    qd, kd, vd, dod = mk(B * L), mk(B * Lkd), mk(B * Lkd), mk(B * L)
    for b, n in enumerate(lengths):
        dod[b * L + n:(b + 1) * L] = 0
    o_d, lse_d = lib.attn_fwd(qd, kd, vd, B, H, L, Lkd, causal, p=p, seed=7, stream_id=3)
    dq_d, dk_d, dv_d = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    o_lo_d = None
    if dtype == torch.bfloat16:
        o_d, lse_d, o_lo_d = lib.attn_fwd(qd, kd, vd, B, H, L, Lkd, causal, p=p, seed=7, stream_id=3, want_lo=True)
    lib.attn_bwd(qd, kd, vd, o_d, dod, lse_d, dq_d, dk_d, dv_d, B, H, L, Lkd, causal, p=p, seed=7, stream_id=3, o_lo=o_lo_d)
    pl = _plan(_labels_with(lengths, L), dev)
    T = pl.Tcap
    sel = torch.cat([torch.arange(b * L, b * L + n) for b, n in enumerate(lengths)]).to(dev)
    nT = sel.numel()
    pack = lambda x: torch.cat([x[sel], mk(T - nT)])
    qp, dop = pack(qd), torch.cat([dod[sel], torch.zeros(T - nT, H * 64, device=dev, dtype=dtype)])
    kp, vp_ = (pack(kd), pack(vd)) if causal else (kd, vd)
    o_p, lse_p, lo_p = _varlen_fwd_raw(qp, kp, vp_, pl, Lk, causal, p, lib)
    ulps = 1 if dtype == torch.bfloat16 else 0
    assert _close_ulp(o_p[:nT], o_d[sel], ulps)
    assert torch.equal(o_p[nT:], torch.zeros_like(o_p[nT:]))
    if lo_p is not None:
        assert torch.equal(lo_p[nT:], torch.zeros_like(lo_p[nT:]))
    lse_dp = lse_d.permute(1, 0, 2).reshape(H, B * L)[:, sel]
    assert torch.allclose(lse_p[:, :nT], lse_dp, rtol=0, atol=0 if ulps == 0 else 1e-6)
    assert torch.equal(lse_p[:, nT:], torch.zeros_like(lse_p[:, nT:]))
    dq_p, dk_p, dv_p = _nan(qp.shape, dtype, dev), _nan(kp.shape, dtype, dev), _nan(vp_.shape, dtype, dev)
    lib.attn_bwd_varlen(qp, kp, vp_, o_p, dop, lse_p, dq_p, dk_p, dv_p, pl, H, Lk, causal, p=p, seed=7, stream_id=3, o_lo=lo_p)
    assert _close_ulp(dq_p[:nT], dq_d[sel], ulps)
    assert torch.equal(dq_p[nT:], torch.zeros_like(dq_p[nT:]))
    if causal:
        assert _close_ulp(dk_p[:nT], dk_d[sel], ulps) and _close_ulp(dv_p[:nT], dv_d[sel], ulps)
        assert torch.equal(dk_p[nT:], torch.zeros_like(dk_p[nT:])) and torch.equal(dv_p[nT:], torch.zeros_like(dv_p[nT:]))
    else:
        assert _close_ulp(dk_p, dk_d, ulps) and _close_ulp(dv_p, dv_d, ulps)


def _model(variant, dtype, dev, **over):
    from mrmt3.synthetic import T5_SMALL
    cfg = dict(T5_SMALL, **over)
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        return T5ForConditionalGeneration(cfg, compute_dtype=dtype).load_golden().to(dev)
    if variant == "segmem_v2":
        from models.t5_segmem_v2 import T5SegMemV2
        return T5SegMemV2(cfg, 1, 64, compute_dtype=dtype).load_golden().to(dev)
    from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
    return T5SegMemV2WithPrev(cfg, 1, 64, compute_dtype=dtype).load_golden().to(dev)


def _engine_grads(m, mel, lab, prev, packed):
    """One forward + backward of the engine (p = 0): (loss, {name: grad})."""
    from mrmt3 import lib
    eng = m.engine
    m.flat.ensure_grads()
    pl = _plan(lab.cpu(), mel.device) if packed else None
    targets = lab.reshape(-1) if pl is None else pl.targets
    kw = dict(training=False, need_grad=True, pack=pl)
    if eng.dt == torch.bfloat16:
        dec, tape = eng.forward(mel, lab, None if prev is None else prev.clone(), want_logits=False, **kw)
        loss, dl = lib.lmhead_cross_entropy(dec, eng.W("lm_head"), targets, want_grad=True, grad_dtype=torch.bfloat16)
    else:
        logits, tape = eng.forward(mel, lab, None if prev is None else prev.clone(), **kw)
        loss, dl = lib.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets, want_grad=True, grad_dtype=torch.float32)
    m.flat.G.zero_()
    eng.backward(tape, dl)
    torch.cuda.synchronize()
    return float(loss.item()), {k: m.flat.grad(k).detach().float().cpu().clone() for k in m.flat.shapes}


def _oracle(variant, mel, lab, prev):
    from mrmt3.synthetic import T5_SMALL, golden_weights
    from oracle import t5_ref
    torch.set_num_threads(8)
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in golden_weights(T5_SMALL, 0 if variant == "t5" else 1).items()}
    logits = t5_ref.forward_logits(sd, T5_SMALL, mel, lab, variant=variant, targets_prev=None if prev is None else prev.clone())
    loss = t5_ref.ce_loss(logits, lab)
    loss.backward()
    return float(loss.item()), {k: v.grad for k, v in sd.items()}


def _rel(a, b):
    return float((a - b).norm() / b.norm()) if b.norm() > 0 else float(a.norm())


VARIANTS = ["t5", "segmem_v2", "segmem_v2_with_prev"]


@pytest.fixture(scope="module")
def model_inputs():
    from mrmt3.synthetic import synth_mel, synth_labels
    B = 2
    mel = torch.from_numpy(synth_mel(B))
    lab = torch.from_numpy(synth_labels(B, 256, full=False, seed=777, mean_len=120))
    prev = torch.from_numpy(synth_labels(B, 256, full=False, seed=999, mean_len=120))
    return mel, lab, prev


@pytest.mark.parametrize("variant", VARIANTS)
def test_packed_fp32_engine_equals_dense_and_oracle(dev, model_inputs, variant):
    """fp32 engine, p = 0: packed loss and every gradient tensor against the dense engine (|d loss| <= 1e-6, rel-L2 <= 2e-6)
    and against the oracle's autograd (the bounds of test_fp32_gradients_match_oracle: loss 2e-5, rel-L2 1e-4)."""
    mel, lab, prev = model_inputs
    prev = prev if variant == "segmem_v2_with_prev" else None
    m = _model(variant, torch.float32, dev)
    args = (mel.to(dev), lab.to(dev), None if prev is None else prev.to(dev))
    ld, gd = _engine_grads(m, *args, packed=False)
    lp, gp = _engine_grads(m, *args, packed=True)
    lo, go = _oracle(variant, mel, lab, prev)
    assert abs(lp - ld) <= 1e-6 and abs(lp - lo) < 2e-5, (lp, ld, lo)
    for k in gd:
        if gd[k].norm() == 0:
            assert gp[k].norm() < 1e-7, k
            continue
        assert _rel(gp[k], gd[k]) <= 2e-6, (k, _rel(gp[k], gd[k]))
        if go.get(k) is not None and go[k].norm() > 0:
            assert _rel(gp[k], go[k]) < 1e-4, (k, _rel(gp[k], go[k]))


@pytest.mark.parametrize("variant", VARIANTS)
def test_packed_bf16_engine_within_dense_bf16_noise(dev, model_inputs, variant):
    """bf16 engine: loss within 1e-3 of the oracle; per gradient tensor, the packed rel-L2 against fp32 autograd is at most
    1.5 x the dense bf16 engine's + 1e-4."""
    mel, lab, prev = model_inputs
    prev = prev if variant == "segmem_v2_with_prev" else None
    m = _model(variant, torch.bfloat16, dev)
    args = (mel.to(dev), lab.to(dev), None if prev is None else prev.to(dev))
    _, gd = _engine_grads(m, *args, packed=False)
    lp, gp = _engine_grads(m, *args, packed=True)
    lo, go = _oracle(variant, mel, lab, prev)
    assert abs(lp - lo) < 1e-3, (lp, lo)
    for k, r in go.items():
        if r is None or r.norm() == 0:
            continue
        assert _rel(gp[k], r) <= 1.5 * _rel(gd[k], r) + 1e-4, (k, _rel(gp[k], r), _rel(gd[k], r))


def _batch(dev, B=3, L=192, seed=0, full=False):
    from mrmt3.synthetic import synth_mel, synth_labels
    mel = torch.from_numpy(synth_mel(B, seed=seed + 1)).to(dev)
    lab = torch.from_numpy(synth_labels(B, L, full=full, seed=seed + 2, mean_len=40)).to(dev)
    return mel, lab


def test_trainer_packed_fp32_steps_equal_dense(dev):
    """Three fp32 optimizer steps, p = 0, packed against dense: every parameter within rel-L2 1e-5.  (The gradients agree to
    2e-6 — test_packed_fp32_engine_equals_dense_and_oracle — but the packed step sums its weight gradients over fewer rows, in
    another order, and AdamW divides every element by its own RMS: for elements whose gradient is near zero a difference of
    1e-7 becomes a difference of a whole update.  Measured 2.2e-6 on the worst tensor.)"""
    from mrmt3.trainer import Trainer
    data = [_batch(dev, seed=s) for s in range(3)]
    P = {}
    for packed in (False, True):
        m = _model("t5", torch.float32, dev, dropout_rate=0.0)
        tr = Trainer(m, lr=1e-3, graph=False, pack_targets=packed)
        for mel, lab in data:
            tr.train_step(mel, lab)
        torch.cuda.synchronize()
        P[packed] = {k: m.flat.master(k).detach().cpu().clone() for k in m.flat.shapes}
    for k in P[False]:
        assert _rel(P[True][k], P[False][k]) <= 1e-5, k


def test_trainer_packed_graph_replay_and_signatures(dev):
    """bf16, dropout 0.1: the packed step replayed from graphs equals the eager packed step bit for bit; two batches of
    different Tcap each capture and replay; a full-length batch runs the dense kernels only; with p = 0.1 the packed loss is
    finite and the same in two runs."""
    from mrmt3 import lib
    from mrmt3.trainer import Trainer
    a = _batch(dev, seed=0)                       # Tcap 256 or 512 (granule 256 at B*L = 576)
    b = (a[0], a[1].clone())
    b[1][:, :150] = 5                             # 150-token rows: T = 450 -> Tcap 512 (a: Tcap 256)
    b[1][:, 150:] = -100
    order = [a, b, a, b, a, b, a, b]
    runs = {}
    for use_graph in (False, True, True):
        m = _model("t5", torch.bfloat16, dev)
        tr = Trainer(m, lr=1e-3, graph=use_graph, pack_targets=True)
        caps = {tr.pack_capacity(x[1]) for x in (a, b)}
        assert len(caps) == 2 and None not in caps
        losses = [float(tr.train_step(*x).item()) for x in order]
        torch.cuda.synchronize()
        assert all(np.isfinite(losses))
        if use_graph:
            assert sum(1 for s in tr._graphs if len(s) == 6) == 2          # both packed signatures captured
        runs.setdefault(use_graph, []).append((losses, m.flat.P.clone()))
        tr.close()
    (le, pe), = runs[False]
    for lg, pg in runs[True]:
        assert le == lg and torch.equal(pe, pg)
    # a full-length batch: dense path, no varlen launch
    m = _model("t5", torch.bfloat16, dev)
    tr = Trainer(m, lr=1e-3, graph=False, pack_targets=True)
    full = _batch(dev, seed=4, full=True)
    assert tr.pack_capacity(full[1]) is None
    lib.dispatch_counts(reset=True)
    tr.train_step(*full)
    torch.cuda.synchronize()
    c = lib.dispatch_counts()
    assert c["attn_fwd_varlen"] == 0 and c["attn_bwd_varlen"] == 0 and c["attn_fwd"] > 0
    lib.dispatch_counts(reset=True)
    tr.train_step(*a)
    torch.cuda.synchronize()
    c = lib.dispatch_counts()
    assert c["attn_fwd_varlen"] > 0 and c["attn_bwd_varlen"] > 0
