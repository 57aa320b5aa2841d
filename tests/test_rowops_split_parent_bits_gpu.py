"""The row, embedding, loss, optimizer and layout entry points write the bits they wrote before csrc/rowops.hip was split
into rowops.hip, embed.hip, loss.hip, optim.hip and layout.hip, its dtype / width ladders were replaced by mr_dtype /
mr_const (csrc/common.h) and the three lm_head chunk loops by one (loss.hip).  The kernels themselves are the parent's,
instruction for instruction (profiles/r19_rowops_split.txt); what this file pins is the host side: which instantiation,
grid and argument list every known dtype / width / option combination gets.  tests/golden/rowops_split_parent.json holds,
for each case below, the sha256 of every buffer the call wrote as the PARENT commit (named in the file) wrote it on an MI355X.

How the golden was recorded: the parent commit's csrc/ was built into a library of its own, a script loaded it in place of
the tree's (MRMT3_TOOL_LIB: the C ABI and the Python binding did not change), ran `run_case(name, dev)` for every name in
CASES and dumped {"parent": <commit>, "cases": {name: result}} as JSON.

Every call goes to the C ABI directly.  Inputs are seeded normal values from numpy's default_rng on the host.  Every output
buffer is allocated with GUARD rows behind it, filled with a sentinel, checked to be untouched and hashed with the rest.
The shapes are the smallest that take each branch: rows = 5 leaves a norm workgroup (4 waves, one row each) with idle
waves, rows = 70 gives the norm backward 18 workgroups the last of which owns two rows; the cross-entropy cases score two
of their five rows, so at most two workgroups add into the f64 loss and the sum does not depend on their arrival order
(the lm_head cases keep their scored rows inside two workgroups for the same reason)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowops_split_parent.json")
BF, F32 = torch.bfloat16, torch.float32
GUARD, SENT = 3, -7.25
WIDTHS = (256, 512, 1024, 2048)
NAMES = {F32: "f32", BF: "bf16", None: "null"}


def _so():
    from mrmt3 import lib
    return lib, lib.load()


def _dt(dtype):
    return 1 if dtype == BF else 0


def _rand(rng, shape, dtype, dev, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dev).to(dtype).contiguous()


def _out(rows, cols, dtype, dev):
    """[rows + GUARD, cols] of the sentinel: the call may write the first `rows` rows"""
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=dev)


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _h(t, rows):
    """sha256 of the whole buffer, guard rows included, which must still hold the sentinel"""
    torch.cuda.synchronize()
    assert bool((t[rows:] == SENT).all()), "guard rows were written"
    return _sha(t)


def _ok(rc, so):
    assert rc == 0, so.mrmt3_last_error()


# ---- add + RMS norm -------------------------------------------------------------------------------------------------------
def case_norm_fwd(dev, cols, ty, tn, p=0.0, out_drop=0):
    lib, so = _so()
    rows, rng = 5, np.random.default_rng(1901)
    x0, w = _rand(rng, (rows, cols), F32, dev), _rand(rng, (cols,), F32, dev)
    y = None if ty is None else _rand(rng, (rows, cols), ty, dev)
    x1, xn, rstd = _out(rows, cols, F32, dev), _out(rows, cols, tn, dev), _out(rows, 1, F32, dev)
    _ok(so.mrmt3_add_rmsnorm_fwd(lib._p(x0), lib._p(y), _dt(ty), lib._p(w), 1e-6, lib._p(x1), lib._p(xn), _dt(tn), lib._p(rstd),
                                 rows, cols, p, 20251, None, 11, 12, out_drop, lib._stream()), so)
    return {"x1": _h(x1, rows), "xn": _h(xn, rows), "rstd": _h(rstd, rows)}


def case_norm_bwd(dev, rows, cols, tg, tri, tro, dw="reduce", p=0.0, out_drop=0, want_dy=True):
    """dw: "reduce" (dw and a workspace: partial rows, then the reduce), "defer" (a workspace alone: the partial rows are
    left in it), "none" (neither)."""
    lib, so = _so()
    rng = np.random.default_rng(1902)
    dxn, x1 = _rand(rng, (rows, cols), tg, dev), _rand(rng, (rows, cols), F32, dev)
    dres = None if tri is None else _rand(rng, (rows, cols), tri, dev)
    rstd, w = _rand(rng, (rows,), F32, dev).abs() + 0.5, _rand(rng, (cols,), F32, dev)
    dx1 = _out(rows, cols, tro, dev)
    dy = _out(rows, cols, BF, dev) if want_dy else None
    dwv = _out(cols, 1, F32, dev)
    dwv[:cols] = _rand(rng, (cols, 1), F32, dev)
    n_ws = int(so.mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, cols))
    ws = torch.zeros(n_ws, dtype=torch.uint8, device=dev) if dw != "none" else None
    _ok(so.mrmt3_add_rmsnorm_bwd(lib._p(dxn), _dt(tg), lib._p(dres), _dt(tri), lib._p(x1), lib._p(rstd), lib._p(w), lib._p(dx1),
                                 _dt(tro), lib._p(dy), lib._p(dwv) if dw == "reduce" else None, rows, cols, p, 20251, None, 11,
                                 12, out_drop, lib._p(ws), n_ws if ws is not None else 0, lib._stream()), so)
    r = {"dx1": _h(dx1, rows), "dw": _h(dwv, cols)}
    if want_dy:
        r["dy"] = _h(dy, rows)
    if dw == "defer":
        n_part = int(so.mrmt3_add_rmsnorm_bwd_partial_rows(rows))
        torch.cuda.synchronize()
        r["partial"] = _sha(ws[:n_part * cols * 4])
    return r


# ---- gated GELU ---------------------------------------------------------------------------------------------------------
def case_geglu(dev, dff, t, p=0.0):
    lib, so = _so()
    rows, rng = 3, np.random.default_rng(1903)
    h, dg = _rand(rng, (rows, 2 * dff), t, dev), _rand(rng, (rows, dff), t, dev)
    g, dh = _out(rows, dff, t, dev), _out(rows, 2 * dff, t, dev)
    _ok(so.mrmt3_geglu_fwd(lib._p(h), lib._p(g), rows, dff, _dt(t), p, 20251, None, 13, lib._stream()), so)
    _ok(so.mrmt3_geglu_bwd(lib._p(h), lib._p(dg), lib._p(dh), rows, dff, _dt(t), p, 20251, None, 13, lib._stream()), so)
    return {"g": _h(g, rows), "dh": _h(dh, rows)}


# ---- embed.hip ------------------------------------------------------------------------------------------------------------
def case_addpos(dev, t):
    lib, so = _so()
    rows, seq_len, d, rng = 6, 3, 8, np.random.default_rng(1904)
    src, pos = _rand(rng, (rows, d), t, dev), _rand(rng, (seq_len + 1, d), F32, dev)
    x = _out(rows, d, F32, dev)
    _ok(so.mrmt3_addpos_fwd(lib._p(src), _dt(t), lib._p(pos), lib._p(x), rows, seq_len, d, 1, 0.1, 20251, None, 14,
                            lib._stream()), so)
    return {"x": _h(x, rows)}


def case_dropmask_cast(dev, t, p):
    lib, so = _so()
    dx = _rand(np.random.default_rng(1905), (3, 4), F32, dev)
    out = _out(3, 4, t, dev)
    _ok(so.mrmt3_dropmask_cast(lib._p(dx), lib._p(out), _dt(t), 12, p, 20251, None, 15, lib._stream()), so)
    return {"out": _h(out, 3)}


# ---- layout.hip -----------------------------------------------------------------------------------------------------------
def case_cast(dev, ti, to):
    lib, so = _so()
    src = _rand(np.random.default_rng(1906), (3, 4), ti, dev)
    out = _out(3, 4, to, dev)
    _ok(so.mrmt3_cast(lib._p(src), _dt(ti), lib._p(out), _dt(to), 12, lib._stream()), so)
    return {"out": _h(out, 3)}


def case_transpose(dev, ti, to):
    lib, so = _so()
    src = _rand(np.random.default_rng(1907), (33, 65), ti, dev)
    out = _out(65, 33, to, dev)
    _ok(so.mrmt3_transpose(lib._p(src), _dt(ti), lib._p(out), _dt(to), 33, 65, lib._stream()), so)
    return {"out": _h(out, 65)}


def case_transpose_batched(dev):
    """64 x 64 at offset 0 (16 bytes per lane) and 9 x 7 behind it (single elements), one tile each"""
    lib, so = _so()
    n = 64 * 64 + 9 * 7
    src = _rand(np.random.default_rng(1908), (n, 1), BF, dev)
    dst = _out(n, 1, BF, dev)
    tab = np.zeros(2, dtype=[("src", "<i8"), ("dst", "<i8"), ("rows", "<i4"), ("cols", "<i4")])
    tab[0], tab[1] = (0, 0, 64, 64), (4096, 4096, 9, 7)
    tab_dev = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    starts = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    _ok(so.mrmt3_transpose_batched(lib._p(src), lib._p(dst), lib._p(tab_dev), lib._p(starts), 2, 2, lib._stream()), so)
    return {"dst": _h(dst, n)}


# ---- loss.hip -------------------------------------------------------------------------------------------------------------
def _ce_inputs(dev, V, weighted):
    rng = np.random.default_rng(1909)
    logits = _rand(rng, (5, V), F32, dev, scale=3.0)
    second = 1140 if weighted else V - 3                     # 1140: inside [1135, 1262], the weighted range
    targets = torch.tensor([-100, 7, -100, second, -100], dtype=torch.int64, device=dev)
    return logits, targets


def _denom(lib, so, targets, weighted, acc, at):
    den = ctypes.c_void_p(acc.data_ptr() + at)
    _ok(so.mrmt3_ce_count(lib._p(targets), targets.numel(), weighted, 1135, 1262, den, lib._stream()), so)
    return den


def case_ce(dev, V, td, reg, weighted=0):
    lib, so = _so()
    rows = 5
    logits, targets = _ce_inputs(dev, V, weighted)
    acc = torch.zeros(3, dtype=torch.float64, device=dev)     # [objective, nll, denom (f32 in its first 4 bytes)]
    den = _denom(lib, so, targets, weighted, acc, 16)
    dl = None if td is None else _out(rows, V, td, dev)
    if reg:
        _ok(so.mrmt3_ce_fwd_bwd_reg(lib._p(logits), lib._p(targets), den, 0.1, 1e-4, lib._p(acc), lib._p(dl), _dt(td), rows, V,
                                    weighted, 1135, 1262, 0.5, lib._stream()), so)
    else:
        _ok(so.mrmt3_ce_fwd_bwd(lib._p(logits), lib._p(targets), den, lib._p(acc), lib._p(dl), _dt(td), rows, V, weighted, 1135,
                                1262, 0.5, lib._stream()), so)
    torch.cuda.synchronize()
    r = {"loss": _sha(acc[:2].float()), "denom": _sha(acc[2:])}
    if dl is not None:
        r["dlogits"] = _h(dl, rows)
    return r


def case_token_logprob(dev, V):
    lib, so = _so()
    rows = 5
    logits = _rand(np.random.default_rng(1910), (rows, V), F32, dev, scale=3.0)
    targets = torch.tensor([3, -100, V - 1, V, 0], dtype=torch.int64, device=dev)       # -100: 0.0; V: out of range, NaN
    out = _out(rows, 1, F32, dev)
    _ok(so.mrmt3_token_logprob(lib._p(logits), lib._p(targets), lib._p(out), rows, V, -100, lib._stream()), so)
    return {"out": _h(out, rows)}


def _lmhead_inputs(dev, t):
    rng = np.random.default_rng(1911)
    dec, w = _rand(rng, (10, 512), t, dev), _rand(rng, (1536, 512), t, dev, scale=0.05)
    # scored: rows 1, 2 and 9 — the first and the last workgroup of the one-chunk launch, one row per chunk of four otherwise
    targets = torch.tensor([-100, 7, 1140, -100, -100, -100, -100, -100, -100, 1530], dtype=torch.int64, device=dev)
    return dec, w, targets


def case_lmhead_ce(dev, chunk, reg, td=BF):
    lib, so = _so()
    rows, V, d = 10, 1536, 512
    dec, w, targets = _lmhead_inputs(dev, BF)
    acc = torch.zeros(3, dtype=torch.float64, device=dev)
    den = _denom(lib, so, targets, 1, acc, 16)
    dl = _out(rows, V, td, dev)
    n_ws = min(rows, chunk) * V * 4
    ws = torch.zeros(n_ws, dtype=torch.uint8, device=dev)
    if reg:
        _ok(so.mrmt3_lmhead_ce_fwd_bwd_reg(lib._p(dec), d, lib._p(w), d, lib._p(targets), den, 0.1, 1e-4, lib._p(acc), lib._p(dl),
                                           _dt(td), rows, V, d, 1, 1135, 1262, 0.5, lib._p(ws), n_ws, chunk, lib._stream()), so)
    else:
        _ok(so.mrmt3_lmhead_ce_fwd_bwd(lib._p(dec), d, lib._p(w), d, lib._p(targets), den, lib._p(acc), lib._p(dl), _dt(td), rows,
                                       V, d, 1, 1135, 1262, 0.5, lib._p(ws), n_ws, chunk, lib._stream()), so)
    torch.cuda.synchronize()
    return {"loss": _sha(acc[:2].float()), "dlogits": _h(dl, rows)}


def case_lmhead_logprob(dev, chunk, t):
    lib, so = _so()
    rows, V, d = 10, 1536, 512
    dec, w, targets = _lmhead_inputs(dev, t)
    out = _out(rows, 1, F32, dev)
    n_ws = min(rows, chunk) * V * 4
    ws = torch.zeros(n_ws, dtype=torch.uint8, device=dev)
    _ok(so.mrmt3_lmhead_logprob(lib._p(dec), d, lib._p(w), d, lib._p(targets), lib._p(out), rows, V, d, _dt(t), lib._p(ws), n_ws,
                                chunk, lib._stream()), so)
    return {"out": _h(out, rows)}


# ---- optim.hip ------------------------------------------------------------------------------------------------------------
def case_adamw_flat(dev, with_stat):
    lib, so = _so()
    rng = np.random.default_rng(1912)
    p, m, v = _out(3, 4, F32, dev), _out(3, 4, F32, dev), _out(3, 4, F32, dev)
    p[:3], m[:3], v[:3] = _rand(rng, (3, 4), F32, dev), _rand(rng, (3, 4), F32, dev, 0.1), _rand(rng, (3, 4), F32, dev).square()
    g = _rand(rng, (3, 4), F32, dev)
    shadow = _out(3, 4, BF, dev)
    lr = torch.tensor([1e-3], dtype=F32, device=dev)
    step = torch.tensor([4], dtype=torch.int32, device=dev)
    stat = torch.tensor([2.0, 0.625, 0.0], dtype=F32, device=dev) if with_stat else None
    for _ in range(2):
        _ok(so.mrmt3_adamw_step(lib._p(p), lib._p(g), lib._p(m), lib._p(v), None, 12, None, 0, 0, lib._p(lr), lib._p(step), 0.9,
                                0.999, 1e-8, 0.01, 1.0 / 3.0, 0.0, lib._p(stat), 0.5 if with_stat else 0.0, lib._p(shadow),
                                lib._stream()), so)
    torch.cuda.synchronize()
    return {"p": _h(p, 3), "m": _h(m, 3), "v": _h(v, 3), "shadow": _h(shadow, 3), "step": _sha(step)}


def case_grad_norm(dev):
    lib, so = _so()
    g = _rand(np.random.default_rng(1913), (12,), F32, dev)
    ws = lib.grad_norm_workspace(dev)
    stat = _out(3, 1, F32, dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    _ok(so.mrmt3_grad_norm(lib._p(g), 12, None, 0, 1.0 / 3.0, 0.25, 1, lib._p(ws), ws.numel(), lib._p(stat), lib._p(skipped),
                           lib._stream()), so)
    torch.cuda.synchronize()
    return {"stat": _h(stat, 3), "skipped": _sha(skipped)}


def _cases():
    c = {}
    pairs = [(a, b) for a in (F32, BF) for b in (F32, BF)]
    # norm forward: every width with the f32 and the bf16 pair, every pair at 512, y null, dropout with out_drop
    for cols in WIDTHS:
        for ty, tn in (pairs if cols == 512 else [(F32, F32), (BF, BF)]):
            c["norm-fwd-%d-y-%s-xn-%s" % (cols, NAMES[ty], NAMES[tn])] = (case_norm_fwd, (cols, ty, tn))
    c["norm-fwd-512-y-null-xn-bf16"] = (case_norm_fwd, (512, None, BF))
    c["norm-fwd-512-y-null-xn-f32"] = (case_norm_fwd, (512, None, F32))
    c["norm-fwd-512-drop-outdrop"] = (case_norm_fwd, (512, BF, BF, 0.1, 1))
    # norm backward: f32 residual at every width, the six bf16-residual combinations at 512, dres null, the three dw forms
    for rows in (5, 70):
        for cols in WIDTHS:
            for tg in (F32, BF):
                c["norm-bwd-r%d-%d-g-%s-res-f32" % (rows, cols, NAMES[tg])] = (case_norm_bwd, (rows, cols, tg, F32, F32))
        for tg in (F32, BF):
            for tri, tro in ((BF, BF), (BF, F32), (F32, BF)):
                c["norm-bwd-r%d-512-g-%s-res-%s-%s" % (rows, NAMES[tg], NAMES[tri], NAMES[tro])] = \
                    (case_norm_bwd, (rows, 512, tg, tri, tro))
        c["norm-bwd-r%d-512-dres-null" % rows] = (case_norm_bwd, (rows, 512, BF, None, F32))
        c["norm-bwd-r%d-512-dres-null-dx1-bf16" % rows] = (case_norm_bwd, (rows, 512, BF, None, BF))
    c["norm-bwd-r70-1024-dres-null"] = (case_norm_bwd, (70, 1024, F32, None, F32))
    c["norm-bwd-r70-512-defer"] = (case_norm_bwd, (70, 512, BF, BF, BF, "defer"))
    c["norm-bwd-r70-512-no-dw"] = (case_norm_bwd, (70, 512, BF, BF, BF, "none"))
    c["norm-bwd-r5-256-no-dw-no-dy"] = (case_norm_bwd, (5, 256, F32, F32, F32, "none", 0.0, 0, False))
    c["norm-bwd-r70-512-drop-outdrop"] = (case_norm_bwd, (70, 512, BF, BF, BF, "reduce", 0.1, 1))
    for t in (F32, BF):
        for dff in (8, 264):
            c["geglu-%d-%s" % (dff, NAMES[t])] = (case_geglu, (dff, t))
        c["geglu-264-%s-drop" % NAMES[t]] = (case_geglu, (264, t, 0.1))
        c["addpos-%s" % NAMES[t]] = (case_addpos, (t,))
        for p in (0.0, 0.1):
            c["dropmask-cast-%s-p%g" % (NAMES[t], p)] = (case_dropmask_cast, (t, p))
    for ti, to in pairs:
        c["cast-%s-%s" % (NAMES[ti], NAMES[to])] = (case_cast, (ti, to))
        c["transpose-%s-%s" % (NAMES[ti], NAMES[to])] = (case_transpose, (ti, to))
    c["transpose-batched-64x64-9x7"] = (case_transpose_batched, ())
    # cross-entropy: V = 512 .. 2048 take the wave kernel, 520 the general one
    for V in (512, 1024, 1536, 2048, 520):
        for td in (BF, F32, None):
            for reg in (0, 1):
                c["ce%s-%d-%s" % ("-reg" if reg else "", V, NAMES[td])] = (case_ce, (V, td, reg))
    for V in (1536, 1520):
        for reg in (0, 1):
            c["ce%s-%d-bf16-weighted" % ("-reg" if reg else "", V)] = (case_ce, (V, BF, reg, 1))
    for V in (520, 1536):
        c["token-logprob-%d" % V] = (case_token_logprob, (V,))
    for chunk in (4, 16):
        for reg in (0, 1):
            c["lmhead-ce%s-chunk%d" % ("-reg" if reg else "", chunk)] = (case_lmhead_ce, (chunk, reg))
        c["lmhead-ce-chunk%d-f32-grad" % chunk] = (case_lmhead_ce, (chunk, 0, F32))
        for t in (BF, F32):
            c["lmhead-logprob-%s-chunk%d" % (NAMES[t], chunk)] = (case_lmhead_logprob, (chunk, t))
    c["adamw-flat"] = (case_adamw_flat, (False,))
    c["adamw-flat-stat"] = (case_adamw_flat, (True,))
    c["grad-norm-12"] = (case_grad_norm, ())
    return c


CASES = _cases()


def run_case(name, dev):
    fn, args = CASES[name]
    out = fn(dev, *args)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_the_golden_names_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_equal_the_parent(dev, golden, name):
    assert run_case(name, dev) == golden["cases"][name]
