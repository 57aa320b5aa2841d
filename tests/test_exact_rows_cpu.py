"""The constructions, references and bounds of tests/test_exact_rows_gpu.py, proven without a GPU (tests/_exact_rows.py):
every exactness claim holds (values representable, sums below 2^24, the p = 0.5 keep scale equal to 2), a torch-f32
restatement of each kernel's formula in torch's own summation order meets every bound, and every seeded fault, down to one
wrong element of a 40001 x 512 output, is caught.  The faults are applied on the CPU; no kernel is touched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402
import _exact_rows as er  # noqa: E402


def _caught(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ---- A ------------------------------------------------------------------------------------------------------------------------

def test_position_code_is_exact_in_bf16_and_tells_misrouted_elements_apart():
    for rows, cols in er.TRANSPOSE_SHAPES + [(259, 1028), (2048, 512)]:
        x = er.position_coded(rows, cols)
        assert torch.equal(x.bfloat16().float(), x) and float(x.abs().max()) <= 256 * 16
        k = (x / torch.pow(2.0, (torch.arange(rows) % 8 - 3).float())[:, None])
        assert torch.equal(k, k.round()) and float(k.abs().max()) <= 256
        w = min(cols, er.CODE_MOD)
        assert all(x[r, :w].unique().numel() == w for r in (0, rows - 1))               # a row's columns are all different
        if rows > 1:
            assert float((x[1:] == x[:-1]).float().mean()) < 0.01                       # neighbouring rows differ (but at 0)
    n = er.EW_SIZES[1]
    x = er.position_coded_flat(n)
    assert torch.equal(x.bfloat16().float(), x)
    for off in er.MISROUTES:
        if off < n:
            assert float((x[off:] == x[:-off]).float().mean()) < 0.01, off                # an element moved by `off` differs


def test_one_wrong_element_of_40001_by_512_is_caught_by_the_equality_check():
    x = er.position_coded(40001, 512)
    y = x.clone()
    ex.assert_equal_everywhere(y, x, "copy")
    y[40000, 509] = x[40000, 508]                             # the neighbour's value in the last quad of the tail row
    assert ex.rel_l2(y, x) < 1e-5                             # invisible to a tensor norm at 4e-3 or 1e-5
    _caught(ex.assert_equal_everywhere, y, x, "copy")
    _caught(er.assert_same_bits, y.bfloat16(), x.bfloat16(), "copy")


def test_bf16_special_values_round_as_the_issue_says_on_the_cpu():
    v = er.bf16_special_values()
    b = v.bfloat16()
    assert float(b[0]) == 1.0 and float(b[1]) == 1.015625 and float(b[2]) == -1.0 and float(b[3]) == -1.015625
    assert float(b[4]) == 1.0078125 and float(b[5]) == 1.0078125 and float(b[6]) == 1.0                 # a tie +- one ulp
    assert float(b[7]) == float(v[7]) and float(b[9]) == float(v[7]) and float(b[10]) == -float(v[7])      # 3.39e38: below half way
    assert float(b[11]) == float("inf") and float(b[16]) == float("inf") and float(b[17]) == float("-inf")  # 3.4e38: above it
    assert er.bits16(b[13:15]).tolist() == [0, -32768] and bool(torch.isnan(b[15]))
    q = er.quads_with_each_value_at_each_position(v)
    assert q.shape == (72, 4) and all(torch.equal(q[4 * i + j, j].view(torch.int32), v[i].view(torch.int32)) for i in range(18) for j in range(4))
    assert er.check_bf16_conversion(q.bfloat16(), q, "cpu") == "rne"
    wrong = q.bfloat16()
    wrong[1, 1] = 1.0078125                                   # the tie rounded away from even
    _caught(er.check_bf16_conversion, wrong, q, "tie")
    wrong = q.bfloat16()
    wrong[4 * 14, 0] = 0.0                                    # -0 lost its sign
    _caught(er.check_bf16_conversion, wrong, q, "sign of zero")
    s = er.quads_with_each_value_at_each_position(er.bf16_subnormal_values())
    assert bool(((s.abs() < er.F32_MIN_NORMAL) & (s != 0)).any(1).all())
    assert er.check_bf16_conversion(s.bfloat16(), s, "cpu", subnormal=True) == "rne"
    flushed = torch.where(s.abs() < er.F32_MIN_NORMAL, torch.copysign(torch.zeros_like(s), s), s).bfloat16()
    assert er.check_bf16_conversion(flushed, s, "flushed", subnormal=True) == "flushed"
    _caught(er.check_bf16_conversion, (-flushed.float()).bfloat16(), s, "wrong sign", subnormal=True)


def test_transpose_batched_tables_take_the_paths_they_name():
    for shift, even in ((0, True), (2, True), (1, False)):
        recs, total = er.trb_table(shift)
        assert [(r, c) for _, _, r, c in recs] == er.TRB_SHAPES
        spans = sorted((d, d + r * c) for _, d, r, c in recs)
        assert spans[0][0] >= er.TRB_GAP and spans[-1][1] + er.TRB_GAP <= total
        assert all(b[0] - a[1] >= er.TRB_GAP for a, b in zip(spans, spans[1:]))
        for s, d, r, c in recs:
            assert s % 8 == shift and d % 8 == shift and (r % 8, c % 8) == (0, 0) and ((s | d) % 2 == 0) == even
    # with shift 0 a matrix runs 16-byte tiles inside AND overhanging tiles (64 does not divide 136, 72 or 200)
    assert any(r > 64 and r % 64 and c >= 64 for r, c in er.TRB_SHAPES) and (64, 64) in er.TRB_SHAPES


def test_keep_scale_at_one_half_is_exactly_two_and_integer_operands_stay_exact():
    keep, scale = er.keep_mask_torch(4096, 0.5, 1234, 5)
    assert scale == 2.0 and 0.45 < float(keep.float().mean()) < 0.55
    keep7, _ = er.keep_mask_torch(4096, 0.5, 1234, 5, step=7)
    assert not torch.equal(keep, keep7)
    from oracle import dropout_ref as dr
    for pp, seed, stream, step in ((0.5, 1234, 5, None), (0.5, 2 ** 40 + 77, 13, 7), (0.1, 2 ** 63 + 5, 200, 1000003), (0.3, 9, 0, 0)):
        want, scale = dr.keep_mask(40001 * 4, pp, seed, stream, step)
        got, gscale = er.keep_mask_torch(40001 * 4, pp, seed, stream, step)
        assert gscale == float(scale) and torch.equal(got, torch.from_numpy(want))


def test_token_ids_and_labels_for_restate_the_shift_right_rule():
    eff = torch.tensor([5, 0, 9, 0, 3])
    for shift in (False, True):
        lab, start = er.labels_for(eff, shift, pad_id=0)
        assert torch.equal(er.token_ids(lab, 5, shift, start, 0, 10), eff)
        assert (not shift) or bool((lab == -100).any())
    assert er.token_ids(torch.tensor([50, -3]), 2, False, 0, 0, 10).tolist() == [9, 0]


# ---- B ------------------------------------------------------------------------------------------------------------------------

def test_embedding_gradient_sums_stay_below_2_pow_24_and_layouts_hit_the_chunk_boundaries():
    assert max(er.eb_sum_bound(r, 2.0) for r in er.EB_ROWS_LIST) < ex.EXACT_F32
    assert [v % 32 for v in er.EB_VOCABS] == [0, 15]
    ids = er.eb_ids("runs", 257, 1391, 0).sort().values
    _, counts = ids.unique_consecutive(return_counts=True)
    assert counts.tolist()[:5] == er.EB_RUNS
    edges = torch.cumsum(counts, 0).tolist()
    assert edges[0] == er.EB_CHUNK and edges[1] == 3 * er.EB_CHUNK and edges[3] == 4 * er.EB_CHUNK     # runs end ON boundaries
    assert er.eb_ids("three", 255, 1536, 0).unique().tolist() == [0, 769, 1535]
    assert er.eb_ids("one", 33, 1536, 0).unique().numel() == 1
    for rows in er.EB_ROWS_LIST:
        assert er.eb_ids("runs", rows, 1391, 1).numel() == rows
    # the f32 sum equals the fp64 sum in any order
    rows, d = 16401, 4
    dx = ex.rand_ints((rows, d), -er.EB_DX, er.EB_DX, torch.float32, "cpu", 1)
    ids = er.eb_ids("one", rows, 1536, 0)
    want = torch.zeros(1536, d, dtype=torch.float64).index_add_(0, ids, dx.double())
    fwd = torch.zeros(1536, d).index_add_(0, ids, dx)
    rev = torch.zeros(1536, d).index_add_(0, ids.flip(0), dx.flip(0))
    assert torch.equal(fwd.double(), want) and torch.equal(rev.double(), want)


def test_norm_weight_gradient_sums_are_exact_and_one_dropped_addend_of_40001_rows_is_caught():
    assert er.dw_sum_bound(40001, 2.0) <= er.EXACT_HALVES and er.dw_sum_bound(40001, 1.0, passes=2) <= er.EXACT_HALVES
    assert er.dw_sum_bound(40001) == 40001 * 4 * 16 + 100 < ex.EXACT_F32
    x1, rstd, dxn, dw0 = er.dw_case(40001, 512, "cpu", 3)
    assert float(x1.abs().max()) == er.DW_X1 and float(dxn.abs().max()) == er.DW_G and set(rstd.unique().tolist()) == set(er.DW_RSTD)
    ref = er.dw_reference(x1, rstd, dxn, dw0)
    assert torch.equal(ref.float().double(), ref)
    f32 = dw0.clone()
    for r0 in range(0, 40001, 4099):                                   # another order, f32 all the way
        f32 += ((dxn[r0:r0 + 4099] * (x1[r0:r0 + 4099] * rstd[r0:r0 + 4099, None]))).sum(0)
    ex.assert_equal_everywhere(f32, ref.float(), "dw in f32")
    keep, scale = er.keep_mask_torch(40001 * 512, 0.5, 9, 3)
    refd = er.dw_reference(x1, rstd, dxn, dw0, keep, scale)
    assert torch.equal(refd.float().double(), refd) and not torch.equal(refd, ref)
    dxn2 = dxn.clone()
    r, c = 40000, 511
    dxn2[r, c] = 0.0 if float(dxn[r, c] * x1[r, c]) != 0 else 1.0     # one addend of the last row dropped (or invented)
    x1[r, c] = x1[r, c] if float(x1[r, c]) != 0 else 1.0
    _caught(ex.assert_equal_everywhere, er.dw_reference(x1, rstd, dxn2, dw0).float(), er.dw_reference(x1, rstd, dxn, dw0).float(), "dw")
    # dx1 of the integer case (w = 1) is exact in f32 as well: f32 arithmetic in the kernel's order equals fp64
    for cols in er.DW_COLS:
        x1, rstd, dxn, _ = er.dw_case(37, cols, "cpu", cols)
        w = torch.ones(cols)
        got = er.norm_bwd_restated(dxn, torch.zeros_like(x1), x1, rstd, w)
        ex.assert_equal_everywhere(got, er.dx1_integer_reference(x1, rstd, dxn, w).float(), "integer dx1")
        assert torch.equal(got.double(), er.dx1_integer_reference(x1, rstd, dxn, w))


# ---- C ------------------------------------------------------------------------------------------------------------------------

def _norm_check_fwd(x0, y, w, got, bf16=False):
    ref = er.norm_fwd_reference(x0, y, w)
    x1, xn, rstd = got
    a = er.check_bound("x1", x1, ref["x1"], ref["x1_tol"])
    b = er.check_bound("rstd", rstd, ref["rstd"], ref["rstd_tol"])
    c = er.check_bound("xn", xn, ref["xn"], er.with_bf16(ref["xn_tol"], ref["xn"]) if bf16 else ref["xn_tol"])
    return max(a, b, c)


@pytest.mark.parametrize("rows,cols", [(r, 512) for r in er.NORM_ROWS] + [(5, c) for c in er.NORM_COLS if c != 512])
def test_norm_restatement_meets_the_bounds_and_the_seeded_faults_do_not(rows, cols):
    for first in (range(0, er.NORM_KINDS, rows) if rows < er.NORM_KINDS else [0]):
        x0, y, w, dxn, dres = er.norm_case(rows, cols, first)
        assert float(w.min()) < 0 and bool((w == 0).any()) and w.unique().numel() >= cols - 1
        for yy in (y, None):
            got = er.norm_fwd_restated(x0, yy, w)
            assert _norm_check_fwd(x0, yy, w, got) <= 1.0
            assert _norm_check_fwd(x0, yy, w, (got[0], got[1].bfloat16(), got[2]), bf16=True) <= 1.0
        x1, xn, rstd = er.norm_fwd_restated(x0, y, w)
        ref, tol = er.norm_bwd_reference(dxn, dres, x1, rstd, w)
        got = er.norm_bwd_restated(dxn, dres, x1, rstd, w)
        assert er.check_bound("dx1", got, ref, tol) <= 1.0
        assert er.check_bound("dx1 bf16", got.bfloat16(), ref, er.with_bf16(tol, ref)) <= 1.0
        assert bool(torch.isfinite(ref).all())
    if rows >= er.NORM_KINDS:
        x0, y, w, dxn, dres = er.norm_case(rows, cols, 0)
        assert float((x0[0] + y[0]).abs().max()) == 0.0                                   # the all-zero row
        ref = er.norm_fwd_reference(x0, y, w)
        assert abs(float(ref["rstd"][0]) - er.NORM_EPS ** -0.5) < 1e-6 and float(ref["xn"][0].abs().max()) == 0.0
        for fault in ("eps_outside", "mean_cols_minus_4"):
            _caught(_norm_check_fwd, x0, y, w, er.norm_fwd_restated(x0, y, w, fault=fault))
        x1, xn, rstd = er.norm_fwd_restated(x0, y, w)
        ref, tol = er.norm_bwd_reference(dxn, dres, x1, rstd, w)
        _caught(er.check_bound, "dx1", er.norm_bwd_restated(dxn, dres, x1, rstd, w, drop_dot_row=rows - 1), ref, tol)


def test_one_wrong_element_of_a_40001_by_512_norm_output_is_caught():
    rows, cols = 40001, 512
    g = torch.Generator().manual_seed(4)
    x1, w = torch.randn(rows, cols, generator=g), 1 + 0.1 * torch.randn(cols, generator=g)
    dxn, dres = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    rstd = torch.rsqrt((x1 * x1).mean(1) + er.NORM_EPS)
    ref, tol = er.norm_bwd_reference(dxn, dres, x1, rstd, w)
    got = er.norm_bwd_restated(dxn, dres, x1, rstd, w)
    assert er.check_bound("dx1", got, ref, tol) <= 1.0
    got[40000, 3] *= 1 + 2.0 ** -16                                    # one element of the tail row, off in its 16th bit
    assert ex.rel_l2(got, ref) < 1e-6
    _caught(er.check_bound, "dx1", got, ref, tol)


@pytest.mark.parametrize("dff", er.GEGLU_DFF)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_geglu_restatement_meets_the_bounds_and_the_seeded_faults_do_not(dff, dtype):
    h, dg = er.geglu_case(dff, dtype)
    a = h[:, :dff].float()
    assert float(a.abs().max()) == float(torch.tensor(1e4).to(dtype)) and all(bool((a == v).any()) for v in (0.0, 20.0, -100.0)) and a.numel() >= 64 * 96 + 9
    assert bool((a.abs() == (1e-30 if dtype == torch.float32 else float(torch.tensor(1e-30).bfloat16()))).any())
    b = h[:, dff:].float().abs()
    assert 2.0 ** -3 * 0.99 <= float(b.min()) and float(b.max()) <= 2.0 ** 3 * 1.01 and b.unique().numel() > 0.9 * b.numel() * (1 if dtype == torch.float32 else 0.01)
    ref = er.geglu_reference(h, dg)
    assert bool(torch.isfinite(ref["dh"]).all() and torch.isfinite(ref["dh_tol"]).all())
    bf = dtype == torch.bfloat16
    tol = lambda k: er.with_bf16(ref[k + "_tol"], ref[k]) if bf else ref[k + "_tol"]

    def check(fault=None):
        g, dh = er.geglu_restated(h, dg, fault)
        ra = er.check_bound("g", g.to(dtype), ref["g"], tol("g"))
        return max(ra, er.check_bound("dh", dh.to(dtype), ref["dh"], tol("dh")))
    assert check() <= 1.0
    for fault in ("k_0447", "erf", "no_q"):
        _caught(check, fault)


@pytest.mark.parametrize("V", er.CE_VOCABS)
@pytest.mark.parametrize("reg", [False, True])
def test_cross_entropy_restatement_meets_the_bounds_and_a_wrong_element_does_not(V, reg):
    lo, hi = (1135, 1262) if V == 1536 else (V // 2, V // 2 + 20)
    opts = dict(eps=er.CE_EPS, z=er.CE_Z) if reg else {}
    for rows in er.CE_ROWS:
        for first in (range(er.CE_KINDS) if rows == 1 else [0]):
            l, t = er.logits_case(rows, V, first, inst=(lo, hi))
            for weighted in (False, True):
                ref = er.ce_reference(l, t, weighted, lo, hi, er.CE_GRAD_SCALE, **opts)
                for block in (False, True):
                    if block and er.ce_wave_kernel_takes(V):
                        continue                                          # the wave kernel never forms exp(l - lse)
                    loss, nll, dl = er.ce_restated(l, t, weighted, lo, hi, er.CE_GRAD_SCALE, block=block, **opts)
                    assert er.check_bound("dlogits", dl, ref["dl"], ref["dl_tol"]) <= 1.0
                    assert abs(loss - ref["loss"]) <= ref["loss_tol"] and abs(nll - ref["nll"]) <= ref["nll_tol"]
                    assert float(dl[~ref["scored"]].abs().max()) == 0.0 if bool((~ref["scored"]).any()) else True
    l, t = er.logits_case(37, V, 0, inst=(lo, hi))
    kinds = torch.arange(37) % er.CE_KINDS
    assert float(l[kinds == 0].min()) > 9e3 and float(l[kinds == 1].max()) < -9e3
    top2 = l.topk(5, 1).values
    assert bool((top2[kinds == 2, 0] - top2[kinds == 2, 1] >= er.CE_MARGIN - 1e-3).all())
    assert bool((top2[kinds == 3, 0] == top2[kinds == 3, 3]).all() and (top2[kinds == 3, 3] > top2[kinds == 3, 4]).all())
    assert bool((l[kinds == 4].argmax(1) == 0).all() and (l[kinds == 5].argmax(1) == V - 1).all())
    assert bool((t == 0).any() and (t == V - 1).any() and (t[4::5] == -100).all() and ((t >= lo) & (t <= hi)).any())
    cols = er.ce_tie_columns(V)
    assert len({(c // 4) % 64 for c in cols}) == 4                                                   # four lanes
    assert V < 1024 or er.ce_wave_kernel_takes(V) or len({(c // 4) % 256 // 64 for c in cols}) >= 3      # waves of ce_kernel
    ref = er.ce_reference(l, t, True, lo, hi, er.CE_GRAD_SCALE, **opts)
    _, _, dl = er.ce_restated(l, t, True, lo, hi, er.CE_GRAD_SCALE, block=not er.ce_wave_kernel_takes(V), **opts)
    r = 6                                                                 # a Gaussian row: one probability off in its 12th bit
    c = int(l[r].argmax())
    dl[r, c] += abs(float(dl[r, c])) * 2.0 ** -12
    _caught(er.check_bound, "dlogits", dl, ref["dl"], ref["dl_tol"])


def test_token_logprob_restatement_meets_the_bound():
    for V in er.TLP_VOCABS:
        for rows in er.TLP_ROWS:
            for first in (range(er.CE_KINDS) if rows == 1 else [0, 3]):
                l, t = er.logits_case(rows, V, first, ignore_every=0)
                if rows > 1:
                    t[rows - 1] = -100
                ref, tol = er.logprob_reference(l, t)
                mx = l.max(1, keepdim=True).values
                got = (l.gather(1, t.clamp(min=0)[:, None]) - mx)[:, 0] - torch.log(torch.exp(l - mx).sum(1))
                got = torch.where(t == -100, torch.zeros_like(got), got)
                assert er.check_bound("logprob", got, ref, tol) <= 1.0
                if V > 1 and t[0] != -100:
                    got[0] += 2e-5 * max(1.0, abs(float(got[0])))
                    _caught(er.check_bound, "logprob", got, ref, tol)


@pytest.mark.parametrize("step0,n_steps", er.ADAM_SCENARIOS)
def test_adamw_restatement_meets_the_bounds_and_a_seeded_fault_does_not(step0, n_steps):
    n = 4096
    for wd in er.ADAM_WD:
        for gs in er.ADAM_GSCALE:
            p0, m0, v0, grads = er.adam_case(n, step0, n_steps)
            kind = torch.arange(n) % 4
            assert float(grads[:, kind == 1].abs().max()) == 0 and float(grads[0, kind == 2][0]) == er.f32(1e-20) and float(grads[0, kind == 3][0]) == er.f32(1e15)
            ref = er.adam_reference(p0, m0, v0, grads, step0, wd, gs)

            def check(fault=None):
                worst = 0.0
                for (p, m, v), r in zip(er.adam_restated(p0, m0, v0, grads, step0, wd, gs, fault), ref):
                    for name, got in (("p", p), ("m", m), ("v", v)):
                        worst = max(worst, er.check_bound("adamw " + name, got, r[name], r[name + "_tol"]))
                return worst
            assert check() <= 1.0
            _caught(check, "no_bias2" if step0 == 0 else "eps_inside")
            # zero gradients from zero moments: the update is the decay alone, bit for bit
            p = er.adam_restated(p0, m0, v0, grads, step0, wd, gs)[-1][0]
            want = p0.clone()
            for _ in range(n_steps):
                want = want * er.adam_decay_f32(wd)
            assert torch.equal(p[kind == 1], want[kind == 1])
    assert er.f32(0.999) != 0.999 and abs(er.f32(0.999) - 0.999) < 1e-7


def test_check_bound_reports_nan_inf_and_a_zero_bound():
    ref, tol = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    assert er.check_bound("zeros", torch.zeros(8), ref, tol) == 0.0
    assert er.check_bound("minus zero", -torch.zeros(8), ref, tol) == 0.0
    for bad in (float("nan"), float("inf"), 1e-30):
        got = torch.zeros(8)
        got[5] = bad
        _caught(er.check_bound, "bad", got, ref, tol)
