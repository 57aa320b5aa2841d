"""Per-element tests of the row-wise kernels of csrc/rowops.hip, embed.hip, loss.hip, optim.hip and layout.hip on a real MI355X (constructions, fp64 references and bounds:
tests/_exact_rows.py, proven on the CPU by tests/test_exact_rows_cpu.py).

A. Data movement and the f32 -> bf16 conversion: bit-exact on position-coded operands, the dropout mask of every site equal
   to the restatement element by element.
B. Embedding gradient and norm-weight gradient on small integers: equal to the float64 sum.
C. RMSNorm, gated GELU, cross-entropy, token log-probability and AdamW: every element within the bound derived from the
   kernel's operation chain of an fp64 reference.  Each test prints `RATIO <what> <largest error / bound>`.
D. The fused GEGLU kernels at saturated activations: the same bits as the two kernels they replace.
Outputs live in buffers with three sentinel guard rows behind them, which must come back untouched.  No assertion here is a
norm over a whole tensor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402
import _exact_rows as er  # noqa: E402
from test_exact_gpu import SENTINEL, _guarded, _guards_untouched  # noqa: E402  (the sentinel idiom)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


def _report(what, ratio):
    print("RATIO %s %.3f" % (what, ratio))
    assert ratio <= 1.0


def _flat(n, dtype, dev):
    """(buffer, its first n elements) with 3 n sentinel elements behind them."""
    buf, out = _guarded(1, n, dtype, dev)
    return buf, out[0]


def _step(dev, n):
    return None if n is None else torch.tensor([n], device=dev, dtype=torch.int32)


# ---- raw ABI calls into caller-owned outputs ----------------------------------------------------------------------------------------

def _call(name, *args):
    from mrmt3 import lib
    lib._check(getattr(lib.load(), "mrmt3_" + name)(*args, lib._stream()), name)


def _cast(src, out):
    from mrmt3 import lib
    _call("cast", lib._p(src), lib._dt(src), lib._p(out), lib._dt(out), src.numel())


def _dropmask_cast(src, out, p=0.0, seed=0, stream=0, step=None):
    from mrmt3 import lib
    _call("dropmask_cast", lib._p(src), lib._p(out), lib._dt(out), src.numel(), p, seed, lib._p(step), stream)


def _transpose(src, out):
    from mrmt3 import lib
    _call("transpose", lib._p(src), lib._dt(src), lib._p(out), lib._dt(out), src.shape[0], src.shape[1])


def _embed_fwd(labels, table, pos, out, seq_len, shift, start_id=0, pad_id=0, pos_offset=0, p=0.0, seed=0, stream=0, step=None):
    from mrmt3 import lib
    V, d = table.shape
    _call("embed_fwd", lib._p(labels), lib._p(table), lib._p(pos), lib._p(out), labels.numel(), seq_len, d, V, int(shift),
          start_id, pad_id, pos_offset, p, seed, lib._p(step), stream)


def _embed_fwd_packed(ids, tok_pos, table, pos, out, p=0.0, seed=0, stream=0, step=None):
    from mrmt3 import lib
    V, d = table.shape
    _call("embed_fwd_packed", lib._p(ids), lib._p(tok_pos), lib._p(table), lib._p(pos), lib._p(out), ids.numel(), d, V, p, seed,
          lib._p(step), stream)


def _addpos_fwd(src, pos, out, seq_len, pos_offset=0, p=0.0, seed=0, stream=0, step=None):
    from mrmt3 import lib
    rows, d = src.shape
    _call("addpos_fwd", lib._p(src), lib._dt(src), lib._p(pos), lib._p(out), rows, seq_len, d, pos_offset, p, seed, lib._p(step),
          stream)


def _geglu_fwd(h, g, p=0.0, seed=0, stream=0, step=None):
    from mrmt3 import lib
    _call("geglu_fwd", lib._p(h), lib._p(g), h.shape[0], h.shape[1] // 2, lib._dt(h), p, seed, lib._p(step), stream)


def _geglu_bwd(h, dg, dh, p=0.0, seed=0, stream=0, step=None):
    from mrmt3 import lib
    _call("geglu_bwd", lib._p(h), lib._p(dg), lib._p(dh), h.shape[0], h.shape[1] // 2, lib._dt(h), p, seed, lib._p(step), stream)


def _norm_fwd(x0, y, w, x1, xn, rstd, p=0.0, seed=0, stream_y=0, stream_out=0, out_drop=False, step=None):
    from mrmt3 import lib
    rows, cols = x0.shape
    _call("add_rmsnorm_fwd", lib._p(x0), lib._p(y), lib._dt(y) if y is not None else lib.F32, lib._p(w), er.NORM_EPS, lib._p(x1),
          lib._p(xn), lib._dt(xn), lib._p(rstd), rows, cols, p, seed, lib._p(step), stream_y, stream_out, int(out_drop))


def _norm_bwd(dxn, dres, x1, rstd, w, dx1, dy, dw, ws, p=0.0, seed=0, stream_y=0, stream_out=0, out_drop=False, step=None):
    from mrmt3 import lib
    rows, cols = x1.shape
    _call("add_rmsnorm_bwd", lib._p(dxn), lib._dt(dxn), lib._p(dres), lib._dt(dres) if dres is not None else lib.F32, lib._p(x1),
          lib._p(rstd), lib._p(w), lib._p(dx1), lib._dt(dx1), lib._p(dy), lib._p(dw), rows, cols, p, seed, lib._p(step),
          stream_y, stream_out, int(out_drop), lib._p(ws), ws.numel() if ws is not None else 0)


def _norm_ws(rows, cols, dev):
    from mrmt3 import lib
    return torch.empty(lib.load().mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, cols), device=dev, dtype=torch.uint8)


# ---- A. data movement ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", er.EW_SIZES)
def test_cast_and_dropmask_cast_move_every_element_bit_for_bit(dev, n):
    src32 = er.position_coded_flat(n, dev)
    for sdt in (F32, BF16):
        src = src32.to(sdt)
        for odt in (F32, BF16):
            buf, out = _flat(n, odt, dev)
            _cast(src, out)
            ex.assert_equal_everywhere(out, src32.to(odt), "cast %s -> %s n = %d" % (sdt, odt, n))
            _guards_untouched(buf, 1, "cast")
    for odt in (F32, BF16):
        buf, out = _flat(n, odt, dev)
        _dropmask_cast(src32, out)
        ex.assert_equal_everywhere(out, src32.to(odt), "dropmask_cast p = 0 -> %s n = %d" % (odt, n))
        _guards_untouched(buf, 1, "dropmask_cast")


@pytest.mark.parametrize("rows,cols", er.TRANSPOSE_SHAPES)
def test_transpose_moves_every_element_bit_for_bit(dev, rows, cols):
    src32 = er.position_coded(rows, cols, dev)
    for sdt in (F32, BF16):
        for odt in (F32, BF16):
            buf, out = _guarded(cols, rows, odt, dev)
            _transpose(src32.to(sdt), out)
            ex.assert_equal_everywhere(out, src32.t().contiguous().to(odt), "transpose %s -> %s %s" % (sdt, odt, (rows, cols)))
            _guards_untouched(buf, cols, "transpose")


def _run_transpose_batched(dev, shift):
    from mrmt3 import lib
    recs, total = er.trb_table(shift)
    src = torch.full((total,), SENTINEL, device=dev, dtype=BF16)
    for s, _, r, c in recs:
        src[s:s + r * c] = er.position_coded(r, c, dev, BF16).reshape(-1)
    dst = torch.full((total,), SENTINEL, device=dev, dtype=BF16)
    tab = np.zeros(len(recs), dtype=[("src", "<i8"), ("dst", "<i8"), ("rows", "<i4"), ("cols", "<i4")])
    starts, tot = [], 0
    for i, rec in enumerate(recs):
        tab[i] = rec
        starts.append(tot)
        tot += ((rec[2] + 63) // 64) * ((rec[3] + 63) // 64)
    lib.transpose_batched(src, dst, torch.from_numpy(tab.view(np.uint8).copy()).to(dev),
                          torch.tensor(starts, dtype=torch.int32, device=dev), len(recs), tot)
    want = torch.full((total,), SENTINEL, device=dev, dtype=BF16)
    for s, d, r, c in recs:
        want[d:d + r * c] = src[s:s + r * c].view(r, c).t().reshape(-1)
    er.assert_same_bits(dst, want, "transpose_batched at offsets = %d (mod 8): matrices and the gaps between them" % shift)


def test_transpose_batched_16_byte_tiles_with_overhang_then_the_pair_and_the_single_element_path(dev):
    """Table (a): dimensions and offsets are multiples of 8, so whole 64 x 64 tiles move 16 bytes per lane and the tiles that
    overhang (136 x 72, 72 x 200) take the pair path of the SAME matrix.  Table (b): the same matrices at offsets = 2 (mod 8)
    (pairs everywhere), then at odd offsets (single elements).  The sentinel gaps between the destinations stay untouched."""
    for shift in (0, 2, 1):
        _run_transpose_batched(dev, shift)


def test_f32_to_bf16_conversion_of_awkward_values_at_each_position_of_a_quad(dev):
    """Ties both ways, a tie +- one f32 ulp, the largest finite bf16, 3.39e38 (still finite) and 3.4e38 (inf), +-inf, +-0 with
    their sign, NaN, through cast (pack_bf2), dropmask_cast (pack_bf2) and transpose (f2bf): torch's CPU rounding of the
    same f32 bits.  f32 SUBNORMALS: torch rounds them to nearest even like any other value (they become bf16 subnormals);
    a zero of the same sign would be accepted as well.  Measured on the MI355X: round to nearest even, not flushed, on
    all three paths (the test prints what it saw)."""
    for sub, vals in ((False, er.bf16_special_values()), (True, er.bf16_subnormal_values())):
        q = er.quads_with_each_value_at_each_position(vals)
        src = q.to(dev)
        n = src.numel()
        seen = []
        buf, out = _flat(n, BF16, dev)
        _cast(src.reshape(-1), out)
        seen.append(er.check_bf16_conversion(out, q, "cast", sub))
        _guards_untouched(buf, 1, "cast")
        buf, out = _flat(n, BF16, dev)
        _dropmask_cast(src.reshape(-1), out)
        seen.append(er.check_bf16_conversion(out, q, "dropmask_cast", sub))
        buf, out = _guarded(4, q.shape[0], BF16, dev)
        _transpose(src, out)
        seen.append(er.check_bf16_conversion(out, q.t().contiguous(), "transpose", sub))
        _guards_untouched(buf, 4, "transpose")
        if sub:
            print("SUBNORMALS f32 -> bf16 (cast, dropmask_cast, transpose): %s" % seen)


@pytest.mark.parametrize("rows", [1, 5, 259])
def test_embedding_forward_gathers_and_adds_exactly(dev, rows):
    V, maxpos = 1391, 64
    seq_len = 37 if rows == 259 else rows
    g = torch.Generator().manual_seed(rows)
    for d in (4, 512, 1028):
        table = er.position_coded(V, d, dev)
        pos = er.position_coded(maxpos, d, dev).flip(0).contiguous()
        labels = torch.randint(1, V - 1, (rows,), generator=g)
        labels[0] = V - 1
        labels[rows // 2] = 0
        if rows > 3:
            labels[rows - 2], labels[1] = -100, V - 1
        labels = labels.to(dev)
        for shift in (False, True):
            for pos_offset in (0, 11):
                ids = er.token_ids(labels, seq_len, shift, 3, 2, V)
                want = table[ids] + pos[(torch.arange(rows, device=dev) % seq_len) + pos_offset]          # one exact f32 add
                assert torch.equal(want.double(), table[ids].double() + pos[(torch.arange(rows, device=dev) % seq_len) + pos_offset].double())
                buf, out = _guarded(rows, d, F32, dev)
                _embed_fwd(labels, table, pos, out, seq_len, shift, 3, 2, pos_offset)
                what = "embed_fwd rows %d d %d shift %s pos_offset %d" % (rows, d, shift, pos_offset)
                ex.assert_equal_everywhere(out, want, what)
                _guards_untouched(buf, rows, what)
        ids = er.token_ids(labels, seq_len, False, 0, 0, V)
        tok_pos = torch.randint(0, maxpos, (rows,), generator=g).int().to(dev)
        buf, out = _guarded(rows, d, F32, dev)
        _embed_fwd_packed(ids, tok_pos, table, pos, out)
        ex.assert_equal_everywhere(out, table[ids] + pos[tok_pos.long()], "embed_fwd_packed rows %d d %d" % (rows, d))
        _guards_untouched(buf, rows, "embed_fwd_packed")
        for sdt in (BF16, F32):
            src = er.position_coded(rows, d, dev).roll(5, 1).contiguous()
            buf, out = _guarded(rows, d, F32, dev)
            _addpos_fwd(src.to(sdt), pos, out, seq_len, 11)
            ex.assert_equal_everywhere(out, src + pos[(torch.arange(rows, device=dev) % seq_len) + 11], "addpos_fwd %s rows %d d %d" % (sdt, rows, d))
            _guards_untouched(buf, rows, "addpos_fwd")


def _nonzero_code(rows, cols, dev, lo=0.125, hi=8.0):
    return er.position_coded(rows, cols, dev).abs().clamp(lo, hi)


@pytest.mark.parametrize("step", [None, 7])
def test_dropout_mask_of_every_site_equals_the_restatement_element_by_element(dev, step):
    """p = 0.5: the keep scale is exactly 2, so every kept value is exactly twice the undropped one and every dropped one is
    zero, at the FLAT OUTPUT INDEX the restatement names; geglu_fwd, geglu_bwd, embed_fwd, embed_fwd_packed, embed_bwd,
    addpos_fwd, add_rmsnorm_fwd (y site and out_drop site), add_rmsnorm_bwd (out_drop site and dy site)."""
    from mrmt3 import lib
    p, seed, rows = 0.5, 2 ** 40 + 77, 37
    sd = _step(dev, step)

    def keep(n, stream):
        k, scale = er.keep_mask_torch(n, p, seed, stream, step, dev)
        assert scale == 2.0
        return k

    def dropped(undropped, k):
        return torch.where(k.reshape(undropped.shape), 2 * undropped, torch.zeros_like(undropped))

    for dt in (F32, BF16):                                              # ---- gated GELU, dff = 8 and 1024
        for dff in (8, 1024):
            h = _nonzero_code(rows, 2 * dff, dev).to(dt)
            g0, g1 = torch.empty(rows, dff, device=dev, dtype=dt), torch.empty(rows, dff, device=dev, dtype=dt)
            _geglu_fwd(h, g0)
            _geglu_fwd(h, g1, p, seed, 5, sd)
            assert bool((g0 != 0).all())
            ex.assert_equal_everywhere(g1, dropped(g0, keep(rows * dff, 5)), "geglu_fwd mask %s dff %d" % (dt, dff))
            dg = _nonzero_code(rows, dff, dev).roll(3, 1).contiguous().to(dt)
            dh0, dh1 = torch.empty_like(h), torch.empty_like(h)
            k = keep(rows * dff, 6).reshape(rows, dff)
            _geglu_bwd(h, torch.where(k, 2 * dg, torch.zeros_like(dg)), dh0)                 # the mask applied by hand
            _geglu_bwd(h, dg, dh1, p, seed, 6, sd)
            assert float((dh0 != 0).float().mean()) > 0.4
            ex.assert_equal_everywhere(dh1, dh0, "geglu_bwd mask %s dff %d" % (dt, dff))
    V, d, seq_len = 1391, 512, 37                                        # ---- embedding forward / packed / backward, addpos
    table, pos = _nonzero_code(V, d, dev), _nonzero_code(64, d, dev).flip(0).contiguous()
    labels = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(1)).to(dev)
    x0, x1 = torch.empty(rows, d, device=dev), torch.empty(rows, d, device=dev)
    _embed_fwd(labels, table, pos, x0, seq_len, True, 3, 2, 4)
    _embed_fwd(labels, table, pos, x1, seq_len, True, 3, 2, 4, p, seed, 9, sd)
    ex.assert_equal_everywhere(x1, dropped(x0, keep(rows * d, 9)), "embed_fwd mask")
    tok_pos = (torch.arange(rows, device=dev) % 50).int()
    _embed_fwd_packed(labels, tok_pos, table, pos, x0)
    _embed_fwd_packed(labels, tok_pos, table, pos, x1, p, seed, 10, sd)
    ex.assert_equal_everywhere(x1, dropped(x0, keep(rows * d, 10)), "embed_fwd_packed mask")
    dx = ex.rand_ints((rows, d), 1, er.EB_DX, F32, dev, 2)
    dt0 = ex.rand_ints((V, d), -er.EB_START, er.EB_START, F32, dev, 3)
    buf, dtab = _guarded(V, d, F32, dev, dt0)
    lib.embed_bwd(labels, dx, dtab, seq_len, True, 3, 2, p=p, seed=seed, stream_id=9, step=sd)
    ids = er.token_ids(labels, seq_len, True, 3, 2, V)
    want = dt0.double().index_add_(0, ids, dropped(dx, keep(rows * d, 9)).double())
    ex.assert_equal_everywhere(dtab, want.float(), "embed_bwd mask")
    _guards_untouched(buf, V, "embed_bwd")
    for sdt in (BF16, F32):
        src = _nonzero_code(rows, d, dev).roll(7, 1).contiguous().to(sdt)
        _addpos_fwd(src, pos, x0, seq_len, 3)
        _addpos_fwd(src, pos, x1, seq_len, 3, p, seed, 11, sd)
        ex.assert_equal_everywhere(x1, dropped(x0, keep(rows * d, 11)), "addpos_fwd mask %s" % sdt)
    for cols in (512, 2048):                                             # ---- add + norm, forward and backward
        n = rows * cols
        xa = ex.rand_ints((rows, cols), -8, 8, F32, dev, 4)
        w = 1 + 0.1 * torch.randn(cols, device=dev)
        for ydt in (F32, BF16):
            y = ex.rand_ints((rows, cols), 1, 8, ydt, dev, 5)
            x1a, xna, rstd = torch.empty_like(xa), torch.empty_like(xa), torch.empty(rows, device=dev)
            x1b, xnb, rstdb = torch.empty_like(xa), torch.empty_like(xa), torch.empty(rows, device=dev)
            _norm_fwd(xa, y, w, x1a, xna, rstd, p, seed, 12, 13, False, sd)
            ex.assert_equal_everywhere(x1a, xa + dropped(y.float(), keep(n, 12)), "add_rmsnorm_fwd y mask %s cols %d" % (ydt, cols))
            _norm_fwd(xa, y, w, x1b, xnb, rstdb, p, seed, 12, 13, True, sd)
            assert torch.equal(x1b, x1a) and torch.equal(rstdb, rstd) and float((xna != 0).float().mean()) > 0.9
            ex.assert_equal_everywhere(xnb, dropped(xna, keep(n, 13)), "add_rmsnorm_fwd out_drop mask %s cols %d" % (ydt, cols))
        for gdt in (F32, BF16):
            dxn = ex.rand_ints((rows, cols), 1, er.DW_G, gdt, dev, 6)
            dres = torch.randn(rows, cols, device=dev)
            ws = _norm_ws(rows, cols, dev)
            outs = []
            for masked_by_hand in (True, False):
                g = dropped(dxn, keep(n, 13)) if masked_by_hand else dxn
                dx1, dy = torch.empty(rows, cols, device=dev), torch.empty(rows, cols, device=dev, dtype=BF16)
                dw = torch.zeros(cols, device=dev)
                _norm_bwd(g, dres, x1a, rstd, w, dx1, dy, dw, ws, p, seed, 12, 13, not masked_by_hand, sd)
                outs.append((dx1, dy, dw))
            for name, a, b in zip(("dx1", "dy", "dw"), outs[0], outs[1]):
                ex.assert_equal_everywhere(b, a, "add_rmsnorm_bwd out_drop mask: %s %s cols %d" % (name, gdt, cols))
            dx1, dy, _ = outs[1]
            ex.assert_equal_everywhere(dy, dropped(dx1, keep(n, 12)).bfloat16(), "add_rmsnorm_bwd dy mask %s cols %d" % (gdt, cols))


# ---- B. exact sums ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", er.EB_ROWS_LIST)
def test_embedding_gradient_of_small_integers_equals_the_float64_sum(dev, rows):
    from mrmt3 import lib
    p, seed = 0.5, 31
    for d in er.eb_widths(rows):
        dx = ex.rand_ints((rows, d), -er.EB_DX, er.EB_DX, F32, dev, rows + d)
        keep, scale = er.keep_mask_torch(rows * d, p, seed, 4, None, dev)
        assert scale == 2.0
        dropped = dx.double() * keep.reshape(rows, d).double() * scale
        for V in er.EB_VOCABS:
            start = ex.rand_ints((V, d), -er.EB_START, er.EB_START, F32, dev, V + d)
            for layout in ("three", "runs", "one"):
                eff = er.eb_ids(layout, rows, V, rows)
                for shift in (False, True):
                    pad_id = int(eff[rows // 2])
                    labels, start_id = er.labels_for(eff, shift, pad_id)
                    labels = labels.to(dev)
                    assert torch.equal(er.token_ids(labels, rows, shift, start_id, pad_id, V).cpu(), eff)
                    for drop in (False, True):
                        want = start.double().index_add_(0, eff.to(dev), dropped if drop else dx.double())
                        assert float(want.abs().max()) <= er.eb_sum_bound(rows, 2.0 if drop else 1.0) < ex.EXACT_F32
                        buf, dtab = _guarded(V, d, F32, dev, start)
                        lib.embed_bwd(labels, dx, dtab, rows, shift, start_id, pad_id, p=p if drop else 0.0, seed=seed, stream_id=4)
                        what = "embed_bwd rows %d d %d V %d %s shift %s drop %s" % (rows, d, V, layout, shift, drop)
                        ex.assert_equal_everywhere(dtab, want.float(), what)
                        _guards_untouched(buf, V, what)


@pytest.mark.parametrize("rows", er.DW_ROWS)
def test_norm_weight_gradient_of_small_integers_equals_the_float64_sum(dev, rows):
    """dw[c] = sum_r dxn x1 rstd with x1 in [-8, 8], rstd in {1/2, 1, 2}, dxn in [-4, 4]: multiples of 1/2 below 2^23, exact in
    any order.  The immediate form, the deferred form (NormDwBatch) and a second accumulation onto the result (at p = 0: with
    the keep scale of 2, two passes over 40001 rows could leave 2^23); p = 0 and p = 0.5 with out_drop; dx1 (weight of ones) is exact on these operands too and is compared bit for bit."""
    from mrmt3 import lib
    p, seed = 0.5, 5
    for cols in er.dw_cols_for(rows):
        w = torch.ones(cols, device=dev)
        ws = _norm_ws(rows, cols, dev)
        mask = er.keep_mask_torch(rows * cols, p, seed, 8, None, dev)
        assert mask[1] == 2.0
        for gdt in (F32, BF16):
            x1, rstd, dxn, dw0 = er.dw_case(rows, cols, dev, rows + cols, gdt)
            inner = er.dx1_integer_reference(x1, rstd, dxn, w)
            exact_dx1 = torch.equal(inner.float().double(), inner)          # the fma rounds an f32 value: to itself
            for drop in (False, True):
                keep, scale = mask if drop else (None, 1.0)
                once = er.dw_reference(x1, rstd, dxn, dw0, keep, scale)
                what = "add_rmsnorm_bwd rows %d cols %d %s drop %s" % (rows, cols, gdt, drop)
                kw = dict(p=p if drop else 0.0, seed=seed, stream_y=7, stream_out=8, out_drop=drop)
                dbuf, dw = _guarded(1, cols, F32, dev, dw0)
                xbuf, dx1 = _guarded(rows, cols, F32, dev)
                _norm_bwd(dxn, None, x1, rstd, w, dx1, None, dw[0], ws, **kw)                 # immediate
                ex.assert_equal_everywhere(dw[0], once.float(), what + ": dw")
                if exact_dx1 and not drop:
                    ex.assert_equal_everywhere(dx1, inner.float(), what + ": dx1")
                _guards_untouched(xbuf, rows, what + ": dx1")
                if not drop:                                                                  # second accumulation
                    assert er.dw_sum_bound(rows, 1.0, passes=2) <= er.EXACT_HALVES
                    _norm_bwd(dxn, None, x1, rstd, w, dx1, None, dw[0], ws, **kw)
                    twice = er.dw_reference(x1, rstd, dxn, once.float())
                    ex.assert_equal_everywhere(dw[0], twice.float(), what + ": dw, accumulated twice")
                _guards_untouched(dbuf, 1, what + ": dw")
                batch = lib.NormDwBatch()                                                     # deferred
                dbuf, dw = _guarded(1, cols, F32, dev, dw0)
                _norm_bwd(dxn, None, x1, rstd, w, dx1, None, None, batch.site(dw[0], rows, cols), **kw)
                ex.assert_equal_everywhere(dw[0], dw0, what + ": dw before the flush")
                batch.flush()
                ex.assert_equal_everywhere(dw[0], once.float(), what + ": dw, deferred")
                _guards_untouched(dbuf, 1, what + ": dw, deferred")


# ---- C. per element against fp64 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(r, 512) for r in er.NORM_ROWS] + [(5, c) for c in er.NORM_COLS if c != 512])
def test_add_rmsnorm_forward_and_backward_per_element_against_fp64(dev, rows, cols):
    worst = {}

    def upd(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    for first in (range(0, er.NORM_KINDS, rows) if rows < er.NORM_KINDS else [0]):
        x0, y32, w, dxn32, dres32 = er.norm_case(rows, cols, first, device=dev)
        for y in (y32, y32.bfloat16(), None):
            ref = er.norm_fwd_reference(x0, y, w)
            for xdt in (F32, BF16):
                for write_x1 in (True, False):
                    what = "add_rmsnorm_fwd rows %d cols %d first %d y %s xn %s x1 %s" % (
                        rows, cols, first, None if y is None else y.dtype, xdt, write_x1)
                    b1, x1 = _guarded(rows, cols, F32, dev)
                    bn, xn = _guarded(rows, cols, xdt, dev)
                    br, rstd = _guarded(rows, 1, F32, dev)
                    _norm_fwd(x0, y, w, x1 if write_x1 else None, xn, rstd)
                    if write_x1:
                        upd("x1", er.check_bound(what + ": x1", x1, ref["x1"], ref["x1_tol"]))
                    else:
                        _guards_untouched(b1, 0, what + ": x1 not written")
                    upd("rstd", er.check_bound(what + ": rstd", rstd[:, 0], ref["rstd"], ref["rstd_tol"]))
                    upd("xn bf16" if xdt == BF16 else "xn", er.check_bound(what + ": xn", xn, ref["xn"],
                                             er.with_bf16(ref["xn_tol"], ref["xn"]) if xdt == BF16 else ref["xn_tol"]))
                    for buf in (b1, bn, br):
                        _guards_untouched(buf, rows, what)
        x1, xn, rstd = torch.empty_like(x0), torch.empty_like(x0), torch.empty(rows, device=dev)
        _norm_fwd(x0, y32, w, x1, xn, rstd)
        for dxn in (dxn32, dxn32.bfloat16()):
            for dres in (dres32, dres32.bfloat16(), None):
                for odt in (F32, BF16):
                    if (odt == BF16 or (dres is not None and dres.dtype == BF16)) and cols != 512:
                        continue                                       # a bf16 residual gradient exists at the model width only
                    ref, tol = er.norm_bwd_reference(dxn, dres, x1, rstd, w)
                    what = "add_rmsnorm_bwd rows %d cols %d first %d dxn %s dres %s dx1 %s" % (
                        rows, cols, first, dxn.dtype, None if dres is None else dres.dtype, odt)
                    bx, dx1 = _guarded(rows, cols, odt, dev)
                    by, dy = _guarded(rows, cols, BF16, dev)
                    _norm_bwd(dxn, dres, x1, rstd, w, dx1, dy, None, None)
                    upd("dx1 bf16" if odt == BF16 else "dx1",
                        er.check_bound(what + ": dx1", dx1, ref, er.with_bf16(tol, ref) if odt == BF16 else tol))
                    upd("dy bf16", er.check_bound(what + ": dy", dy, ref, er.with_bf16(tol, ref)))
                    _guards_untouched(bx, rows, what + ": dx1")
                    _guards_untouched(by, rows, what + ": dy")
    for k, v in sorted(worst.items()):
        _report("add_rmsnorm rows %d cols %d %s" % (rows, cols, k), v)


@pytest.mark.parametrize("dff", er.GEGLU_DFF)
@pytest.mark.parametrize("dt", [F32, BF16])
def test_geglu_forward_and_backward_per_element_against_fp64(dev, dt, dff):
    h, dg = er.geglu_case(dff, dt, dev)
    rows = h.shape[0]
    ref = er.geglu_reference(h, dg)
    tol = lambda k: er.with_bf16(ref[k + "_tol"], ref[k]) if dt == BF16 else ref[k + "_tol"]
    bg, g = _guarded(rows, dff, dt, dev)
    _geglu_fwd(h, g)
    bh, dh = _guarded(rows, 2 * dff, dt, dev)
    _geglu_bwd(h, dg, dh)
    _guards_untouched(bg, rows, "geglu_fwd")
    _guards_untouched(bh, rows, "geglu_bwd")
    _report("geglu_fwd %s dff %d g" % (dt, dff), er.check_bound("geglu_fwd g", g, ref["g"], tol("g")))
    _report("geglu_bwd %s dff %d dh" % (dt, dff), er.check_bound("geglu_bwd dh", dh, ref["dh"], tol("dh")))


def _ce_raw(logits, targets, dl, weighted, lo, hi, grad_scale, reg):
    """lib.cross_entropy with the gradient in the caller's buffer -> (loss, nll or None) as Python floats (fp64 accumulators)."""
    from mrmt3 import lib
    import ctypes as C
    rows, V = logits.shape
    acc = torch.zeros(3 if reg else 2, device=logits.device, dtype=torch.float64)
    den = C.c_void_p(acc.data_ptr() + (16 if reg else 8))
    _call("ce_count", lib._p(targets), rows, int(weighted), lo, hi, den)
    if reg:
        _call("ce_fwd_bwd_reg", lib._p(logits), lib._p(targets), den, er.CE_EPS, er.CE_Z, lib._p(acc), lib._p(dl), lib._dt(dl), rows,
              V, int(weighted), lo, hi, grad_scale)
        return float(acc[0]), float(acc[1])
    _call("ce_fwd_bwd", lib._p(logits), lib._p(targets), den, lib._p(acc), lib._p(dl), lib._dt(dl), rows, V, int(weighted), lo, hi,
          grad_scale)
    return float(acc[0]), None


def _ce_check(dev, rows, V, first, reg, gdt, weighted, worst):
    lo, hi = (1135, 1262) if V == 1536 else (V // 2, V // 2 + 20)
    l, t = er.logits_case(rows, V, first, device=dev, inst=(lo, hi))
    opts = dict(eps=er.CE_EPS, z=er.CE_Z) if reg else {}
    ref = er.ce_reference(l, t, weighted, lo, hi, er.CE_GRAD_SCALE, grad_bf16=gdt == BF16, **opts)
    what = "cross-entropy rows %d V %d first %d reg %s %s weighted %s" % (rows, V, first, reg, gdt, weighted)
    buf, dl = _guarded(rows, V, gdt, dev)
    loss, nll = _ce_raw(l, t, dl, weighted, lo, hi, er.CE_GRAD_SCALE, reg)
    _guards_untouched(buf, rows, what)
    if bool((~ref["scored"]).any()):
        assert float(dl[~ref["scored"]].abs().max()) == 0.0, what + ": an ignored row's gradient is not exactly zero"
    key = "dlogits bf16" if gdt == BF16 else "dlogits"
    worst[key] = max(worst.get(key, 0.0), er.check_bound(what + ": dlogits", dl, ref["dl"], ref["dl_tol"]))
    r = abs(loss - ref["loss"]) / ref["loss_tol"]
    assert r <= 1.0, (what, "loss", loss, ref["loss"], ref["loss_tol"])
    worst["loss"] = max(worst["loss"], r)
    if reg:
        r = abs(nll - ref["nll"]) / ref["nll_tol"]
        assert r <= 1.0, (what, "nll", nll, ref["nll"], ref["nll_tol"])
        worst["nll"] = max(worst["nll"], r)


@pytest.mark.parametrize("V", er.CE_VOCABS)
@pytest.mark.parametrize("rows", er.CE_ROWS)
def test_cross_entropy_per_element_against_fp64(dev, rows, V):
    worst = dict(loss=0.0, nll=0.0)
    for first in (range(er.CE_KINDS) if rows == 1 else [0]):
        for reg in (False, True):
            for gdt in (F32, BF16):
                for weighted in (False, True):
                    _ce_check(dev, rows, V, first, reg, gdt, weighted, worst)
    for k, v in sorted(worst.items()):
        _report("cross-entropy rows %d V %d %s" % (rows, V, k), v)


def test_cross_entropy_at_24577_rows_where_a_wave_walks_three_rows_and_the_last_walk_is_cut_short(dev):
    rows, V = er.CE_BIG
    assert rows // (4 * 2048) == 3 and rows % 12 != 0                   # loss.hip ce_rows_per_wave
    worst = dict(loss=0.0, nll=0.0)
    _ce_check(dev, rows, V, 0, False, F32, False, worst)
    for k in ("dlogits", "loss"):
        _report("cross-entropy rows %d V %d %s" % (rows, V, k), worst[k])


@pytest.mark.parametrize("V", er.TLP_VOCABS)
def test_token_logprob_per_row_against_fp64_log_softmax(dev, V):
    worst = 0.0
    for rows in er.TLP_ROWS:
        for first in (range(er.CE_KINDS) if rows == 1 else [0, 3]):
            l, t = er.logits_case(rows, V, first, device=dev, ignore_every=0)
            nan_row = None
            if rows > 1:
                t[rows - 1] = -100                                      # an ignored row: exactly 0.0
                nan_row = 2
                l[nan_row, V // 2] = float("nan")                       # a row that holds a NaN: NaN
            buf, out = _guarded(rows, 1, F32, dev)
            _call_token_logprob(l, t, out)
            _guards_untouched(buf, rows, "token_logprob")
            got = out[:, 0]
            ok = torch.ones(rows, dtype=torch.bool, device=dev)
            if nan_row is not None:
                assert bool(torch.isnan(got[nan_row])), "a row that holds a NaN must score NaN"
                assert float(got[rows - 1]) == 0.0
                ok[nan_row] = False
            ref, tol = er.logprob_reference(l[ok], t[ok])
            worst = max(worst, er.check_bound("token_logprob V %d rows %d first %d" % (V, rows, first), got[ok], ref, tol))
    _report("token_logprob V %d" % V, worst)


def _call_token_logprob(l, t, out):
    from mrmt3 import lib
    _call("token_logprob", lib._p(l), lib._p(t), lib._p(out), l.shape[0], l.shape[1], -100)


@pytest.mark.parametrize("n", er.EW_SIZES)
@pytest.mark.parametrize("step0,n_steps", er.ADAM_SCENARIOS)
def test_adamw_per_element_against_torch_adamw_in_float64(dev, step0, n_steps, n):
    from mrmt3 import lib
    worst = dict(p=0.0, m=0.0, v=0.0)
    kind = torch.arange(n, device=dev) % 4
    for wd in er.ADAM_WD:
        for gs in er.ADAM_GSCALE:
            p0, m0, v0, grads = er.adam_case(n, step0, n_steps, dev)
            ref = er.adam_reference(p0, m0, v0, grads, step0, wd, gs)
            bufs = [_guarded(1, n, F32, dev, x) for x in (p0, m0, v0)]
            (p, m, v) = (b[1][0] for b in bufs)
            sbuf, shadow = _flat(n, BF16, dev)
            lr = torch.tensor([er.ADAM["lr"]], device=dev)
            step = torch.tensor([step0], device=dev, dtype=torch.int32)
            zero_p = p0.clone()
            for k in range(n_steps):
                lib.adamw_step(p, grads[k], m, v, lr, step, er.ADAM["beta1"], er.ADAM["beta2"], er.ADAM["eps"], wd, gs, shadow=shadow)
                what = "adamw n %d from step %d, step %d wd %g grad_scale %g" % (n, step0, k + 1, wd, gs)
                for name, got in (("p", p), ("m", m), ("v", v)):
                    worst[name] = max(worst[name], er.check_bound(what + ": " + name, got, ref[k][name], ref[k][name + "_tol"]))
                er.assert_same_bits(shadow, p.bfloat16(), what + ": shadow")
                zero_p = zero_p * er.adam_decay_f32(wd).to(dev)
                ex.assert_equal_everywhere(p[kind == 1], zero_p[kind == 1], what + ": zero gradients leave the decay alone")
            assert int(step) == step0 + n_steps
            for b, _ in bufs:
                _guards_untouched(b, 1, "adamw")
            _guards_untouched(sbuf, 1, "adamw shadow")
    for k, val in worst.items():
        _report("adamw n %d from step %d %s" % (n, step0, k), val)


# ---- D. fused kernels at saturated activations ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,dff,K", [(4096, 1024, 512), (2048 + 72, 1024, 512), (1024, 1024, 512)])
def test_gemm_nt_geglu_fused_equals_the_two_kernels_bitwise_at_saturated_activations(dev, knobs, rows, dff, K):
    """tests/test_kernels_gpu.py test_gemm_nt_geglu_fused_equals_the_two_kernels_bitwise with the projection weights x 20: h
    has a standard deviation near 20 and the GELU is saturated on most elements."""
    from mrmt3 import lib
    g = torch.Generator(device=dev).manual_seed(11)
    step = torch.tensor([7], device=dev, dtype=torch.int32)
    x = torch.randn(rows, K, device=dev, generator=g).bfloat16()
    wi = (torch.randn(2 * dff, K, device=dev, generator=g) * 0.06 * 20).bfloat16()
    for p in (0.0, 0.1):
        kw = dict(p=p, seed=1234, stream_id=5, step=step if p else None)
        h1 = lib.gemm_nt(x, wi)
        g1 = lib.geglu_fwd(h1, **kw)
        assert 15.0 < float(h1.float().std()) < 40.0
        assert float(((h1[:, :dff].float().abs() > 5).float().mean())) > 0.7                   # saturated on most elements
        for fused in ("0", "1"):
            knobs.set("MRMT3_GEGLU_FUSED", fused)
            h, gg = lib.gemm_nt_geglu(x, wi, **kw)
            er.assert_same_bits(h, h1, "gemm_nt_geglu h, MRMT3_GEGLU_FUSED=%s p %g" % (fused, p))
            er.assert_same_bits(gg, g1, "gemm_nt_geglu g, MRMT3_GEGLU_FUSED=%s p %g" % (fused, p))


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("rows", [4096, 1000, 24])
def test_gemm_nt_geglubwd_equals_the_two_kernels_bitwise_at_saturated_activations(dev, knobs, tile, rows):
    """tests/test_gemm_rows_gpu.py test_gemm_nt_geglubwd_equals_the_two_kernels_bitwise with the saved projection h and the
    weights x 20."""
    from mrmt3 import lib
    knobs.set("MRMT3_ROWS_BM", tile)
    d, dff = 512, 1024
    g = torch.Generator(device=dev).manual_seed(41)
    dy = torch.randn(rows, d, device=dev, generator=g).bfloat16()
    wt = (torch.randn(dff, d, device=dev, generator=g) * d ** -0.5 * 20).bfloat16()
    h = (torch.randn(rows, 2 * dff, device=dev, generator=g) * 20).bfloat16()
    step = torch.tensor([5], device=dev, dtype=torch.int32)
    for p in (0.0, 0.1):
        kw = dict(p=p, seed=7, stream_id=17, step=step)
        ref = lib.geglu_bwd(h, lib.gemm_nt(dy, wt, out_dtype=BF16), **kw)
        before = lib.dispatch_counts()["gemm_nt_geglubwd"]
        got = lib.gemm_nt_geglubwd(dy, wt, h, **kw)
        assert lib.dispatch_counts()["gemm_nt_geglubwd"] == before + 1
        er.assert_same_bits(got, ref, "gemm_nt_geglubwd dh rows %d tile %d p %g" % (rows, tile, p))
