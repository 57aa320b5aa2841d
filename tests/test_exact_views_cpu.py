"""The constructions and checkers of tests/test_exact_views_gpu.py, proven without a GPU (tests/_exact_views.py): an NT and a
TN product restated on flat memory (pointer + row stride) pass every check on every listed shape and layout, and each of
seven addressing faults — the ones a kernel can have on a view and not on a contiguous matrix — fails the check meant for
it.  The faults are applied to the emulation; no kernel is touched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402
import _exact_views as xv  # noqa: E402
from test_exact_gpu import SENTINEL  # noqa: E402

DEV = "cpu"


def _nt_case(M, N, K, layout, out_dtype, acc, in_dtype=torch.bfloat16):
    abuf, a = xv.operand((M, K), ex.INT_LO, ex.INT_HI, in_dtype, DEV, 11 * M + K, *xv.margins(layout, "a", in_dtype))
    bbuf, b = xv.operand((N, K), ex.INT_LO, ex.INT_HI, in_dtype, DEV, 13 * N + K, *xv.margins(layout, "b", in_dtype))
    c0 = ex.rand_ints((M, N), ex.C0_LO, ex.C0_HI, torch.float32, DEV, M + N) if acc else None
    cbuf, c = xv.output(M, N, out_dtype, DEV, SENTINEL, *xv.margins(layout, "c", out_dtype), c0=c0)
    ref = a.double() @ b.double().t() + (c0.double() if acc else 0)
    assert float(ref.abs().max()) <= ex.int_sum_bound(K) < ex.EXACT_F32
    return (abuf, a), (bbuf, b), (cbuf, c), ref.to(out_dtype)


def _tn_case(M, N1, N2, layout, acc):
    abuf, a = xv.operand((M, N1), ex.INT_LO, ex.INT_HI, torch.bfloat16, DEV, 3 * M + N1, *xv.margins(layout, "a", torch.bfloat16))
    bbuf, b = xv.operand((M, N2), ex.INT_LO, ex.INT_HI, torch.bfloat16, DEV, 5 * M + N2, *xv.margins(layout, "b", torch.bfloat16))
    c0 = ex.rand_ints((N1, N2), ex.C0_LO, ex.C0_HI, torch.float32, DEV, N1 + N2) if acc else None
    cbuf, c = xv.output(N1, N2, torch.float32, DEV, SENTINEL, *xv.margins(layout, "c", torch.float32), c0=c0)
    ref = a.double().t() @ b.double() + (c0.double() if acc else 0)
    assert float(ref.abs().max()) <= ex.int_sum_bound(M) < ex.EXACT_F32
    return (abuf, a), (bbuf, b), (cbuf, c), ref.float()


def _run(kind, A, B, C, ref, dims, acc, fault, what):
    keep = [(A[0], A[0].clone()), (B[0], B[0].clone())]
    emulate = xv.emulate_nt if kind == "nt" else xv.emulate_tn
    emulate(xv.Mem(*A), xv.Mem(*B), xv.Mem(*C), *dims, accumulate=acc, fault=fault)
    xv.check_product(C[0], C[1], ref, what, SENTINEL, keep)


def test_view_in_is_what_it_says():
    buf, v = xv.view_in(5, 16, torch.bfloat16, DEV, SENTINEL, 8, 24, above=2, below=3)
    assert buf.shape == (10, 48) and v.shape == (5, 16) and v.stride() == (48, 1) and v.data_ptr() == buf[2, 8:].data_ptr()
    assert xv.box_of(buf, v) == (2, 8, 5, 16) and bool((buf == SENTINEL).all())
    assert (v.data_ptr() - buf.data_ptr()) % 16 == 0 and (v.stride(0) * 2) % 16 == 0
    with pytest.raises(AssertionError):
        xv.view_in(5, 16, torch.bfloat16, DEV, 0.0, 4, 24)            # 8 bytes: no kernel takes that view
    for dt in (torch.bfloat16, torch.float32):                        # margins: unequal, A / B / C different, off every tile
        ms = [xv.margins(xv.RAGGED, r, dt) for r in "abc"]
        assert len({sum(m) for m in ms[:2]}) == 2 and all(l != r and l % xv.unit(dt) == 0 and r % xv.unit(dt) == 0 for l, r in ms)
        for w in (128, 256, 384, 512, 1152):
            assert all((w + l + r) % 128 != 0 for l, r in ms)
    assert xv.margins(xv.ENGINE, "a", torch.bfloat16) == (384, 0) and 384 + xv.ENGINE_W == 1152
    assert xv.margins(xv.ENGINE, "c", torch.float32) == (768, 4608) and 768 + xv.ENGINE_W + 4608 == 6144


def test_the_sentinel_equals_no_result_and_every_sum_is_exact():
    worst = max([K for _, _, K in xv.NT_TILE_SHAPES + xv.NT8_SMALL + xv.NT8_BIG + xv.NT_SPLITK + xv.NT_ENGINE] +
                [M for M, _, _ in xv.TN_TILE_SHAPES + xv.TN8_SHAPES + xv.TN_GROUP_SITES])
    assert ex.int_sum_bound(worst) < ex.EXACT_F32
    assert SENTINEL != round(SENTINEL)                                                    # f32 results are integers
    worst_k = max(K for _, _, K in xv.NT_TILE_SHAPES + xv.NT8_SMALL + xv.NT8_BIG + xv.NT_SPLITK + xv.NT_ENGINE)
    assert abs(float(torch.tensor(SENTINEL).bfloat16())) > ex.int_sum_bound(worst_k)      # bf16 results (NT only) are smaller


def test_outside_check_compares_bits_and_names_the_element():
    buf, v = xv.view_in(4, 8, torch.float32, DEV, float("nan"), 4, 12)
    v.fill_(1.0)
    xv.assert_outside_untouched(buf, xv.box_of(buf, v), "nan fill", float("nan"))        # NaN against the same NaN: equal
    buf[xv.ABOVE + 1, 4 + 8 + 2] = 0.0
    with pytest.raises(AssertionError, match=r"\(row, column\) = \(1, 10\)"):
        xv.assert_outside_untouched(buf, xv.box_of(buf, v), "nan fill", float("nan"))
    buf, v = xv.view_in(4, 8, torch.float32, DEV, 0.0, 4, 12)
    buf[0, 0] = -0.0                                                                       # equal as a number, not in bits
    with pytest.raises(AssertionError, match=r"\(row, column\) = \(-2, -4\)"):
        xv.assert_outside_untouched(buf, xv.box_of(buf, v), "zero fill", 0.0)


NT_ALL = xv.NT_TILE_SHAPES + xv.NT8_SMALL + xv.NT8_BIG + xv.NT_SPLITK
TN_ALL = xv.TN_TILE_SHAPES + xv.TN8_SHAPES + xv.TN_GROUP_SITES


@pytest.mark.parametrize("M,N,K", NT_ALL)
def test_fault_free_nt_passes_every_check(M, N, K):
    kinds = [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)]
    for out_dtype, acc in (kinds if M < 4096 else kinds[2:]):          # (the tall shapes once: the emulation is one matmul)
        A, B, C, ref = _nt_case(M, N, K, xv.RAGGED, out_dtype, acc)
        _run("nt", A, B, C, ref, (M, N, K), acc, None, "nt %s" % ((M, N, K),))


@pytest.mark.parametrize("M,N,K", xv.NT_TILE_SHAPES)
def test_fault_free_nt_f32_operands_passes_every_check(M, N, K):
    for acc in (False, True):
        A, B, C, ref = _nt_case(M, N, K, xv.RAGGED, torch.float32, acc, in_dtype=torch.float32)
        _run("nt", A, B, C, ref, (M, N, K), acc, None, "nt f32 %s" % ((M, N, K),))


@pytest.mark.parametrize("M,N,K", xv.NT_ENGINE)
def test_fault_free_nt_passes_in_the_engine_layout(M, N, K):
    for out_dtype, acc in ((torch.bfloat16, False), (torch.float32, True)):
        A, B, C, ref = _nt_case(M, N, K, xv.ENGINE, out_dtype, acc)
        assert A[0].shape[1] == 1152 and C[0].shape[1] == 6144 and xv.box_of(*C)[1] == 768
        _run("nt", A, B, C, ref, (M, N, K), acc, None, "nt engine layout %s" % ((M, N, K),))


@pytest.mark.parametrize("M,N1,N2", TN_ALL)
def test_fault_free_tn_passes_every_check(M, N1, N2):
    for acc in (False, True):
        A, B, C, ref = _tn_case(M, N1, N2, xv.RAGGED, acc)
        _run("tn", A, B, C, ref, (M, N1, N2), acc, None, "tn %s" % ((M, N1, N2),))


# fault -> (the words of the check that must fail, accumulate)
CAUGHT_BY = {
    "base_dropped": ("elements differ", False),              # i.   NaN from left of / above the view
    "ld_is_width": ("elements differ", False),               # ii.  rows drift into the margins
    "ld_swapped": ("elements differ", False),                # iii. A and B buffers have different widths
    "tile_past_n": ("outside the view were written", False),  # iv.  lands right of the view, not in the next row's columns
    "row_past_m": ("outside the view were written", False),   # v.   lands in the rows below
    "zero_times_outside": ("elements differ", False),        # vi.  NaN * 0 = NaN
    "wrong_ldc": ("elements differ", True),                  # vii. the start of every row but the first is another element
}


def test_the_seven_faults_are_the_listed_ones():
    assert set(CAUGHT_BY) == set(xv.FAULTS) and len(xv.FAULTS) == 7


# (in the engine's layout A and B have the same stride, nothing to swap, and 768 columns are whole tiles, no ragged last one)
NOT_IN_ENGINE_LAYOUT = ("ld_swapped", "tile_past_n")


@pytest.mark.parametrize("fault,layout", [(f, "ragged") for f in xv.FAULTS] +
                         [(f, "engine") for f in xv.FAULTS if f not in NOT_IN_ENGINE_LAYOUT])
def test_each_fault_fails_its_check_nt(fault, layout):
    words, acc = CAUGHT_BY[fault]
    M, N, K = (129, 136, 96) if layout == "ragged" else (130, xv.ENGINE_W, xv.ENGINE_W)
    lay = xv.RAGGED if layout == "ragged" else xv.ENGINE
    A, B, C, ref = _nt_case(M, N, K, lay, torch.float32, acc)
    with pytest.raises(AssertionError, match=words):
        _run("nt", A, B, C, ref, (M, N, K), acc, fault, "nt %s" % fault)


@pytest.mark.parametrize("fault", xv.FAULTS)
def test_each_fault_fails_its_check_tn(fault):
    words, acc = CAUGHT_BY[fault]
    M, N1, N2 = 64, 72, 40
    A, B, C, ref = _tn_case(M, N1, N2, xv.RAGGED, acc)
    with pytest.raises(AssertionError, match=words):
        _run("tn", A, B, C, ref, (M, N1, N2), acc, fault, "tn %s" % fault)


def test_a_contiguous_output_hides_the_store_past_n():
    """Why the output has to be a view: on a contiguous [M, N] output with guard rows behind it, the columns a last tile
    stores past N are the first columns of the next row, and that row's own store covers them up (stores in row order)."""
    M, N, K = 9, 136, 32
    a = ex.rand_ints((M, K), ex.INT_LO, ex.INT_HI, torch.float32, DEV, 1)
    b = ex.rand_ints((N, K), ex.INT_LO, ex.INT_HI, torch.float32, DEV, 2)
    ref = a @ b.t()
    buf = torch.full((M + 3, N), SENTINEL)
    flat = buf.reshape(-1)
    for r in range(M):                                       # row by row; the last tile stores 128 columns: 120 past N
        flat[r * N:r * N + xv.TILE_N] = ref[r, :xv.TILE_N]
        tail = torch.zeros(xv.TILE_N)
        tail[:N - xv.TILE_N] = ref[r, xv.TILE_N:]
        flat[r * N + xv.TILE_N:r * N + 2 * xv.TILE_N] = tail
    assert torch.equal(buf[:M - 1], ref[:M - 1])             # every row but the last: the overrun is gone without a trace
    assert not bool((buf[M:] == SENTINEL).all())             # only the last row's overrun reaches a guard row
