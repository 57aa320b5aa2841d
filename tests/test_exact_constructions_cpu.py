"""The constructions and checkers of tests/test_exact_gpu.py, proven without a GPU (tests/_exact.py): the integer GEMM
operands stay below 2^24 in every partial sum, the attention construction's closed forms equal fp64 softmax attention and its
autograd, its score margin holds, and each checker fails on a local fault that the older whole-tensor norms let through.
The faults are applied to reference arrays on the CPU; no kernel is touched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402


# ---- A ------------------------------------------------------------------------------------------------------------------------

def test_integer_gemm_sums_stay_below_2_pow_24():
    for M, N, K in ex.NT_SHAPES + [(ex.NT_STRIDED[0], ex.NT_STRIDED[4], ex.NT_STRIDED[3] - ex.NT_STRIDED[2])]:
        assert ex.int_sum_bound(K) < ex.EXACT_F32, (M, N, K)
    for M, N1, N2 in ex.TN_SHAPES + ex.TN_GROUP_SITES + ex.TN_F32_SHAPES:
        assert ex.int_sum_bound(M) < ex.EXACT_F32, (M, N1, N2)
    assert max(ex.int_sum_bound(K) for _, _, K in ex.NT_SHAPES) == 9 * 2304 + 100
    assert max(ex.int_sum_bound(M) for M, _, _ in ex.TN_SHAPES) == 9 * 65536 + 100
    w = ex.NT_F32_WIDE
    assert ex.int_sum_bound(w["K"], w["a_max"], w["b_max"], 0) < ex.EXACT_F32
    assert w["a_max"] >= 2 ** 11 - 1 > 2 ** 8            # more bits than a bf16 holds: a narrowed operand cannot pass


def test_integer_gemm_reference_is_exact_in_any_order():
    """The same product summed in f32 in two different orders and in fp64 gives the same integers."""
    a = ex.rand_ints((37, 2304), ex.INT_LO, ex.INT_HI, torch.float32, "cpu", 1)
    b = ex.rand_ints((24, 2304), ex.INT_LO, ex.INT_HI, torch.float32, "cpu", 2)
    assert a.min() == ex.INT_LO and a.max() == ex.INT_HI
    ref = a.double() @ b.double().t()
    fwd = torch.zeros(37, 24)
    for k0 in range(0, 2304, 128):
        fwd += a[:, k0:k0 + 128] @ b[:, k0:k0 + 128].t()
    rev = torch.zeros(37, 24)
    for k0 in reversed(range(0, 2304, 96)):
        rev += a[:, k0:k0 + 96] @ b[:, k0:k0 + 96].t()
    assert torch.equal(fwd, ref.float()) and torch.equal(rev, ref.float()) and torch.equal(ref.float().double(), ref)
    assert (ref.abs() > 256).any()                       # bf16 output rounds: the test pins round-to-nearest-even


# ---- B ------------------------------------------------------------------------------------------------------------------------

def _closed_form_vs_autograd(c, B, H, Lq, Lk, causal):
    o, lse, dq, dk, dv = ex.attention_autograd(c.q, c.k, c.v, c.d_o, B, H, Lq, Lk, causal)
    for name, ref in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        dev, i = ex.max_deviation(getattr(c, name), ref)
        assert dev <= 1e-9, (name, dev, i)
    assert (c.lse - lse).abs().max().item() <= 1e-9
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("B,H,Lq,Lk,causal", ex.ATTN_SHAPES)
def test_closed_forms_equal_fp64_attention_and_its_autograd(B, H, Lq, Lk, causal):
    c = ex.attention_case(1, 1, Lq, Lk, causal)
    assert c.margin >= ex.MIN_MARGIN
    _closed_form_vs_autograd(c, 1, 1, Lq, Lk, causal)
    for name in ("q", "k", "v", "d_o"):                  # the inputs are bf16 values
        t = getattr(c, name)
        assert torch.equal(t.bfloat16().float(), t)
    assert set(c.v.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(c.d_o.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert (c.q[:, ex.CODE:] == 0).all() and (c.dq[:, :ex.CODE] == 0).all() and (c.dk[:, ex.CODE:] == 0).all()
    for name in ("o", "dq", "dk", "dv"):                 # every step of every output is a multiple of 1/2
        t = getattr(c, name) * 2
        assert torch.equal(t, t.round()), name


def test_closed_form_lse_in_fp64():
    hd = ex.attention_head(300, 300, True, torch.Generator().manual_seed(3))
    _, lse, _, _, _ = ex.attention_autograd(hd["q"], hd["k"], hd["v"], hd["d_o"], 1, 1, 300, 300, True)
    assert (hd["lse"] - lse[0, 0]).abs().max().item() <= 1e-9
    assert set(torch.exp(hd["lse"] - ex.GAIN * ex.CODE).round().tolist()) == {1.0, 2.0}


def test_margin_of_every_listed_shape():
    for B, H, Lq, Lk, causal in ex.ATTN_SHAPES + [(1, 1, n, n, True) for n in ex.VARLEN_LENGTHS if n] + \
            [(1, 1, 37, ex.VARLEN_CROSS_KEYS, False)]:
        book, margin = ex.codebook((Lk + 1) // 2)
        assert margin >= ex.MIN_MARGIN, (Lk, margin)
        if Lk > 1:                                       # the margin the builder returns is the one the scores have
            hd = ex.attention_head(min(Lq, 64), Lk, False, torch.Generator().manual_seed(Lk))
            s = hd["q"] @ hd["k"].t()
            top = s.max(1, keepdim=True).values
            assert (top == ex.GAIN * ex.CODE).all()
            assert (top - s.masked_fill(s == top, float("-inf")).max(1, keepdim=True).values).min().item() >= margin


@pytest.mark.parametrize("cross_keys", [0, ex.VARLEN_CROSS_KEYS])
def test_varlen_closed_forms(cross_keys):
    H = 2
    c = ex.varlen_case(tuple(ex.VARLEN_LENGTHS), H, cross_keys)
    T = sum(ex.VARLEN_LENGTHS)
    assert c.q.shape == (T, H * 64) and c.lse.shape == (H, T)
    q0 = k0 = 0
    for n in ex.VARLEN_LENGTHS:
        Lk = cross_keys or n
        if Lk == 0:
            continue
        sl_q, sl_k = slice(q0, q0 + n), slice(k0, k0 + Lk)
        if n:
            o, lse, dq, dk, dv = ex.attention_autograd(c.q[sl_q], c.k[sl_k], c.v[sl_k], c.d_o[sl_q], 1, H, n, Lk, cross_keys == 0)
            for name, ref, sl in (("o", o, sl_q), ("dq", dq, sl_q), ("dk", dk, sl_k), ("dv", dv, sl_k)):
                assert ex.max_deviation(getattr(c, name)[sl], ref)[0] <= 1e-9, (name, n)
            assert (c.lse[:, sl_q] - lse[0]).abs().max().item() <= 1e-9
        else:
            assert (c.dk[sl_k] == 0).all() and (c.dv[sl_k] == 0).all()
        q0, k0 = q0 + n, k0 + Lk
    assert q0 == T and k0 == c.k.shape[0]


# ---- checker sensitivity: a local fault fails the new check and passes the old whole-tensor one --------------------------------

def test_one_bf16_ulp_in_one_gemm_element_is_caught():
    M, N, K = 1000, 1152, 512
    a = ex.rand_ints((M, K), ex.INT_LO, ex.INT_HI, torch.float64, "cpu", 3)
    b = ex.rand_ints((N, K), ex.INT_LO, ex.INT_HI, torch.float64, "cpu", 4)
    ref = a @ b.t()
    want = ref.float().bfloat16()
    ex.assert_equal_everywhere(want.clone(), want, "untouched")
    got = want.clone()
    got.view(torch.int16)[617, 333] += 1                                   # one ulp, one element
    assert ex.rel_l2(got, ref) < 4e-3                                      # test_gemm_nt_bf16's bound does not see it
    with pytest.raises(AssertionError, match=r"1 of 1152000 elements differ.*\(617, 333\)"):
        ex.assert_equal_everywhere(got, want, "bf16 GEMM")
    got32 = ref.float().clone()
    got32.view(torch.int32)[999, 1151] += 1                                # f32: one element off by one ulp
    assert ex.rel_l2(got32, ref) < 1e-5
    with pytest.raises(AssertionError):
        ex.assert_equal_everywhere(got32, ref.float(), "f32 GEMM")


def _old_backward_check_passes(c, got):
    return all(ex.rel_l2(got[n], getattr(c, n)) < 2e-2 for n in ("dq", "dk", "dv"))


def _new_check_fails(c, got):
    failed = []
    for n in ("dq", "dk", "dv"):
        try:
            ex.check_elements(n, got[n], getattr(c, n), ex.ATTN_TOL, H=c.H)
        except AssertionError:
            failed.append(n)
    return failed


@pytest.fixture(scope="module")
def causal_case():
    return ex.attention_case(2, 6, 1024, 1024, True)                       # a shape of test_attn_bwd_bf16


def test_swapped_rows_are_caught(causal_case):
    c = causal_case
    norms = c.dk.reshape(-1, c.H, 64)[:, 0].norm(dim=-1)                   # head 0: the two smallest nonzero, different rows
    order = [int(i) for i in norms.argsort() if norms[i] > 0]
    r0 = order[0]
    r1 = next(i for i in order[1:] if not torch.equal(c.dk[i, :64], c.dk[r0, :64]))
    got = {n: getattr(c, n).clone() for n in ("dq", "dk", "dv")}
    got["dk"][[r0, r1], :64] = got["dk"][[r1, r0], :64]
    assert _old_backward_check_passes(c, got)
    assert _new_check_fails(c, got) == ["dk"]


def test_a_key_unmasked_past_the_causal_limit_is_caught(causal_case):
    c, L = causal_case, 1024
    sl = slice(0, 64)                                                      # batch 0, head 0
    hq, hk, hv, hg = c.q[:L, sl], c.k[:L, sl], c.v[:L, sl], c.d_o[:L, sl]
    s = hq.double() @ hk.double().t()
    hidden = (s == ex.GAIN * ex.CODE) & (torch.arange(L)[None, :] > torch.arange(L)[:, None])
    i, j = (int(x) for x in hidden.nonzero()[0])                           # query i's second selected key j > i: masked
    _, _, dq, dk, dv = ex.attention_autograd(hq, hk, hv, hg, 1, 1, L, L, True, unmask=((i, j),))
    got = {n: getattr(c, n).clone() for n in ("dq", "dk", "dv")}
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        got[n][:L, sl] = t.float()
    assert _old_backward_check_passes(c, got)
    assert "dv" in _new_check_fails(c, got)
    # the forward's whole-tensor norm does not see it either (its max|err| bound does: kept, not replaced)
    o = ex.attention_autograd(hq, hk, hv, hg, 1, 1, L, L, True, unmask=((i, j),))[0]
    got_o = c.o.clone()
    got_o[:L, sl] = o.float()
    assert ex.rel_l2(got_o, c.o) < 1e-2
    with pytest.raises(AssertionError, match="row, head, dim"):
        ex.check_elements("o", got_o, c.o, ex.ATTN_TOL, H=c.H)


def test_a_dropped_query_key_contribution_is_caught(causal_case):
    c, L = causal_case, 1024
    hd_q, hd_k, hd_v, hd_g = c.q[:L, :64].double(), c.k[:L, :64].double(), c.v[:L, :64].double(), c.d_o[:L, :64].double()
    s = (hd_q @ hd_k.t()).masked_fill(torch.arange(L)[None, :] > torch.arange(L)[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    i = 700
    j = int(p[i].argmax())
    ds = p * (hd_g @ hd_v.t() - (hd_g * (p @ hd_v)).sum(-1, keepdim=True))
    got = {n: getattr(c, n).clone() for n in ("dq", "dk", "dv")}
    got["dv"][j, :64] -= (p[i, j] * hd_g[i]).float()                       # the pair (i, j) left out of dV and dK
    got["dk"][j, :64] -= (ds[i, j] * hd_q[i]).float()
    assert (p[i, j] * hd_g[i]).abs().max() >= 0.5
    assert _old_backward_check_passes(c, got)
    assert "dv" in _new_check_fails(c, got)


def test_row_bound_sees_a_wrong_small_row_that_the_tensor_norm_does_not():
    """Part C's checker: the late keys of a causal dK have small norms; zeroing one moves the tensor norm by nothing."""
    B, H, L = 1, 2, 300
    q, k, v, d_o = ex.gaussian_attention_inputs(B, H, L, L, "cpu")
    _, _, dq, dk, dv = ex.attention_autograd(q, k, v, d_o, B, H, L, L, True)
    _, _, rk, _ = ex.attention_rounded(q, k, v, d_o, B, H, L, L, True)
    limit = ex.ROW_BOUND_FACTOR * ex.row_errors(rk, dk, H).max().item()
    assert 1e-3 < limit < 0.1, limit
    got = dk.float().bfloat16()
    assert ex.row_errors(got, dk, H).max().item() <= limit                 # a correctly rounded result passes
    rn = dk.reshape(L, H, 64).norm(dim=-1)                                 # the smallest row that is not under the floor
    r, h = divmod(int(rn.masked_fill(rn < 1e-2 * rn.median(), float("inf")).reshape(-1).argmin()), H)
    assert r > L // 2                                                      # a late key, as expected
    got[r, h * 64:(h + 1) * 64] = 0
    assert ex.rel_l2(got, dk) < 2e-2
    e = ex.row_errors(got, dk, H)
    assert e.max().item() > limit and int(e.reshape(-1).argmax()) == r * H + h
