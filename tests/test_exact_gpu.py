"""Element-exact tests of the MFMA GEMM and attention kernels on a real MI355X (constructions and checkers: tests/_exact.py,
proven on the CPU by tests/test_exact_constructions_cpu.py).

A. GEMMs on small-integer operands: every partial sum is an integer below 2^24, so the f32 result is the float64 matmul bit
   for bit whatever the summation order, the K split or the slab reduction — `torch.equal` on the whole output, bf16 output
   equal to the round-to-nearest-even of the exact sum, three guard rows behind every output untouched, and the dispatch
   counters say which kernel ran.
B. Attention on inputs with closed-form O, LSE, dQ, dK, dV: every element within 1/8 of a value whose every real fault (a
   misrouted, dropped, doubled or unmasked (query, key) pair) is a step of at least 1/2.
C. Attention backward on Gaussian inputs, scored per 64-wide row against fp64 autograd, the limit set by an fp64 restatement
   with the kernels' rounding points.
No assertion here is a norm over a whole tensor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3
SENTINEL = -77777.5           # no result equals it: f32 results are integers, bf16 results stay below 9 * 2304 + 100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


def _ran(before, **expected):
    """The dispatch counters moved by exactly `expected` since `before` (families not named: not at all)."""
    from mrmt3 import lib
    after = lib.dispatch_counts()
    moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert moved == {k: v for k, v in expected.items() if v}, (moved, expected)


# ---- A. GEMMs ------------------------------------------------------------------------------------------------------------------

def _guarded(rows, cols, dtype, dev, c0=None):
    """([rows + 3, cols] buffer, its first `rows` rows): output and guard rows hold the sentinel, or the output holds the
    integer start of an accumulate case."""
    buf = torch.full((rows + GUARD, cols), SENTINEL, device=dev, dtype=dtype)
    if c0 is not None:
        buf[:rows] = c0
    return buf, buf[:rows]


def _guards_untouched(buf, rows, what):
    ex.assert_equal_everywhere(buf[rows:], torch.full_like(buf[rows:], SENTINEL), what + ": guard rows")


def _nt_raw(a, b, out, accumulate, ws=None):
    from mrmt3 import lib
    L = lib.load()
    M, K = a.shape
    N = b.shape[0]
    args = (lib._p(a), a.stride(0), lib._p(b), b.stride(0), lib._p(out), out.stride(0), M, N, K, lib._dt(a), lib._dt(out),
            int(accumulate))
    if ws is None:
        lib._check(L.mrmt3_gemm_nt(*args, lib._stream()), "gemm_nt")
    else:
        lib._check(L.mrmt3_gemm_nt_ws(*args, lib._p(ws), ws.numel(), lib._stream()), "gemm_nt_ws")


def _nt_operands(M, N, K, dev, dtype=torch.bfloat16):
    a = ex.rand_ints((M, K), ex.INT_LO, ex.INT_HI, dtype, dev, 11 * M + K)
    b = ex.rand_ints((N, K), ex.INT_LO, ex.INT_HI, dtype, dev, 13 * N + K)
    c0 = ex.rand_ints((M, N), ex.C0_LO, ex.C0_HI, torch.float32, dev, M + N)
    ref = a.double() @ b.double().t()                      # exact: integers far below 2^53
    return a, b, c0, ref


def _nt_three_outputs(a, b, c0, ref, dev, what, expect, ws=None):
    """f32, bf16 and f32-accumulate output of one NT product, each equal to the exact result everywhere; `expect(kind)` are
    the counters one launch must move."""
    from mrmt3 import lib
    M, N = ref.shape
    for kind in ("f32", "bf16", "acc"):
        dt = torch.bfloat16 if kind == "bf16" else torch.float32
        buf, out = _guarded(M, N, dt, dev, c0 if kind == "acc" else None)
        before = lib.dispatch_counts()
        _nt_raw(a, b, out, kind == "acc", ws)
        _ran(before, **expect(kind))
        want = (ref + c0.double()).float() if kind == "acc" else ref.float()
        ex.assert_equal_everywhere(out, want.bfloat16() if kind == "bf16" else want, "%s %s" % (what, kind))
        _guards_untouched(buf, M, "%s %s" % (what, kind))


# shapes the ping-pong kernel takes by default on 256 CUs (csrc/gemm8.hip mrmt3_gemm_nt8_try: M >= 2048, N >= 256, N % 128 == 0,
# K % 128 == 0, tiles in whole waves of workgroups, not the accumulate form); every other listed shape runs round 1's kernel
NT8_SHAPES = {(4097, 512, 1024), (3072, 512, 2048), (3000, 512, 2304), (65536, 512, 1024)}


@pytest.mark.parametrize("M,N,K", ex.NT_SHAPES)
def test_gemm_nt_bf16_integer_operands_bit_exact(dev, knobs, M, N, K):
    a, b, c0, ref = _nt_operands(M, N, K, dev)
    assert float(ref.abs().max()) + 100 <= ex.int_sum_bound(K) < ex.EXACT_F32
    for gemm8 in (1, 0):
        knobs.set("MRMT3_GEMM8", gemm8)
        on8 = lambda kind: gemm8 == 1 and (M, N, K) in NT8_SHAPES and kind != "acc"
        _nt_three_outputs(a, b, c0, ref, dev, "gemm_nt %s MRMT3_GEMM8=%d" % ((M, N, K), gemm8),
                          lambda kind: dict(gemm_nt8=int(on8(kind)), gemm_nt_tile=int(not on8(kind))))
    if (M, N, K) in NT8_SHAPES:                     # the ping-pong kernel's accumulate instantiation (not dispatched by default)
        knobs.set("MRMT3_GEMM8", 1)
        knobs.set("MRMT3_GEMM8_ALL", 1)
        _nt_three_outputs(a, b, c0, ref, dev, "gemm_nt %s MRMT3_GEMM8_ALL=1" % ((M, N, K),), lambda kind: dict(gemm_nt8=1))


def test_gemm_nt_bf16_row_strided_a(dev, knobs):
    rows, ld, c_lo, c_hi, N = ex.NT_STRIDED
    big = ex.rand_ints((rows, ld), ex.INT_LO, ex.INT_HI, torch.bfloat16, dev, 5)
    a = big[:, c_lo:c_hi]
    b = ex.rand_ints((N, c_hi - c_lo), ex.INT_LO, ex.INT_HI, torch.bfloat16, dev, 6)
    c0 = ex.rand_ints((rows, N), ex.C0_LO, ex.C0_HI, torch.float32, dev, 7)
    ref = a.double() @ b.double().t()
    for gemm8 in (1, 0):
        knobs.set("MRMT3_GEMM8", gemm8)
        _nt_three_outputs(a, b, c0, ref, dev, "gemm_nt strided A MRMT3_GEMM8=%d" % gemm8, lambda kind: dict(gemm_nt_tile=1))


@pytest.mark.parametrize("M,N,K", ex.NT_SPLITK_SHAPES)
def test_gemm_nt_split_k_bit_exact(dev, knobs, M, N, K):
    """mrmt3_gemm_nt_ws: split over K through the slab (the default for these shapes) and forced unsplit."""
    from mrmt3 import lib
    a, b, c0, ref = _nt_operands(M, N, K, dev)
    nbytes = int(lib.load().mrmt3_gemm_nt_workspace_bytes(M, N, K, lib._dt(a)))
    assert nbytes > 0, "not a split-K shape any more: pick one that is (csrc/gemm8.hip g8_splitk_plan)"
    wbuf = torch.full((nbytes + 4 * 64,), 0x5A, device=dev, dtype=torch.uint8)
    ws = wbuf[:nbytes]
    _nt_three_outputs(a, b, c0, ref, dev, "gemm_nt_ws split %s" % ((M, N, K),), lambda kind: dict(gemm_nt_splitk=1), ws=ws)
    assert bool((wbuf[nbytes:] == 0x5A).all()), "the split-K slab was overrun"
    knobs.set("MRMT3_GEMM8_SPLITK", 0)
    _nt_three_outputs(a, b, c0, ref, dev, "gemm_nt_ws unsplit %s" % ((M, N, K),),
                      lambda kind: dict(gemm_nt8=int(kind != "acc"), gemm_nt_tile=int(kind == "acc")), ws=ws)


@pytest.mark.parametrize("M,N,K", ex.NT_SHAPES)
def test_gemm_nt_f32_integer_operands_bit_exact(dev, M, N, K):
    """The v_mfma_f32_16x16x4_f32 path."""
    a, b, c0, ref = _nt_operands(M, N, K, dev, torch.float32)
    from mrmt3 import lib
    for kind in ("f32", "acc"):
        buf, out = _guarded(M, N, torch.float32, dev, c0 if kind == "acc" else None)
        before = lib.dispatch_counts()
        _nt_raw(a, b, out, kind == "acc")
        _ran(before, gemm_nt_tile=1)
        ex.assert_equal_everywhere(out, (ref + c0.double()).float() if kind == "acc" else ref.float(), "gemm_nt f32 in, %s" % kind)
        _guards_untouched(buf, M, "gemm_nt f32 in, %s" % kind)


def test_gemm_nt_f32_keeps_every_operand_bit(dev):
    """12-bit integers against 8-bit ones at K = 32: products of 20 bits, sums below 2^24 — exact in f32, out of reach of
    any operand narrowed to bf16 (or to a tf32-like format) on the way into the MFMA."""
    w = ex.NT_F32_WIDE
    M, N, K = w["M"], w["N"], w["K"]
    a = ex.rand_ints((M, K), -w["a_max"], w["a_max"], torch.float32, dev, 21)
    b = ex.rand_ints((N, K), -w["b_max"], w["b_max"], torch.float32, dev, 22)
    ref = a.double() @ b.double().t()
    assert float(ref.abs().max()) < ex.EXACT_F32 and not torch.equal(a.bfloat16().float(), a)
    buf, out = _guarded(M, N, torch.float32, dev)
    _nt_raw(a, b, out, False)
    ex.assert_equal_everywhere(out, ref.float(), "gemm_nt f32, 12-bit operands")
    _guards_untouched(buf, M, "gemm_nt f32, 12-bit operands")


# shapes mrmt3_tn8_plan admits at all (M >= 8192, N1 % 128 == 0, N2 % 64 == 0, both >= 256), and the one among the listed
# shapes it takes by default on 256 CUs (the chip filled, <= 15 % overlap in the shifted last tile)
TN8_ADMISSIBLE = {(8200, 896, 320), (65536, 1152, 512)}
TN8_DEFAULT = {(65536, 1152, 512)}


@pytest.mark.parametrize("M,N1,N2", ex.TN_SHAPES)
def test_gemm_tn_integer_operands_bit_exact(dev, knobs, M, N1, N2):
    from mrmt3 import lib
    a = ex.rand_ints((M, N1), ex.INT_LO, ex.INT_HI, torch.bfloat16, dev, 3 * M + N1)
    b = ex.rand_ints((M, N2), ex.INT_LO, ex.INT_HI, torch.bfloat16, dev, 5 * M + N2)
    c0 = ex.rand_ints((N1, N2), ex.C0_LO, ex.C0_HI, torch.float32, dev, N1 + N2)
    ref = a.double().t() @ b.double()
    assert float(ref.abs().max()) + 100 <= ex.int_sum_bound(M) < ex.EXACT_F32
    modes = [("MRMT3_TN8=1", dict(MRMT3_TN8=1), (M, N1, N2) in TN8_DEFAULT), ("MRMT3_TN8=0", dict(MRMT3_TN8=0), False)]
    if (M, N1, N2) in TN8_ADMISSIBLE - TN8_DEFAULT:
        modes.append(("MRMT3_TN8_ALL=1", dict(MRMT3_TN8=1, MRMT3_TN8_ALL=1), True))
    for name, kn, on8 in modes:
        knobs.unset("MRMT3_TN8_ALL")
        for k_, v_ in kn.items():
            knobs.set(k_, v_)
        for acc in (False, True):
            what = "gemm_tn %s %s accumulate=%d" % ((M, N1, N2), name, acc)
            buf, out = _guarded(N1, N2, torch.float32, dev, c0 if acc else None)
            before = lib.dispatch_counts()
            lib.gemm_tn(a, b, out, accumulate=acc)
            _ran(before, tn8=int(on8), tn_tile=int(not on8))
            ex.assert_equal_everywhere(out, (ref + c0.double()).float() if acc else ref.float(), what)
            _guards_untouched(buf, N1, what)


def test_gemm_tn_grouped_launch_bit_exact(dev):
    """One TnGroup launch over four ragged gradients (token counts off the 128-row unit, shifted last tiles in both
    dimensions), accumulate and overwrite mixed."""
    from mrmt3 import lib
    sites = []
    for i, (M, N1, N2) in enumerate(ex.TN_GROUP_SITES):
        a = ex.rand_ints((M, N1), ex.INT_LO, ex.INT_HI, torch.bfloat16, dev, 100 + i)
        b = ex.rand_ints((M, N2), ex.INT_LO, ex.INT_HI, torch.bfloat16, dev, 200 + i)
        acc = i % 2 == 0
        c0 = ex.rand_ints((N1, N2), ex.C0_LO, ex.C0_HI, torch.float32, dev, 300 + i)
        buf, out = _guarded(N1, N2, torch.float32, dev, c0 if acc else None)
        assert lib.TnGroup.ok(a, b, out)
        sites.append((a, b, buf, out, acc, c0))
    grp = lib.TnGroup()
    for a, b, _, out, acc, _ in sites:
        grp.add(a, b, out, accumulate=acc)
    before = lib.dispatch_counts()
    grp.flush()
    _ran(before, tn_group=1)
    for (M, N1, N2), (a, b, buf, out, acc, c0) in zip(ex.TN_GROUP_SITES, sites):
        ref = a.double().t() @ b.double()
        what = "TnGroup site %s accumulate=%d" % ((M, N1, N2), acc)
        ex.assert_equal_everywhere(out, (ref + c0.double()).float() if acc else ref.float(), what)
        _guards_untouched(buf, N1, what)


@pytest.mark.parametrize("M,N1,N2", ex.TN_F32_SHAPES)
def test_gemm_tn_f32_integer_operands_bit_exact(dev, M, N1, N2):
    """Contiguous operands, then strided views of wider buffers: nothing outside the output view may change."""
    from mrmt3 import lib
    abuf = ex.rand_ints((M, N1 + 5), ex.INT_LO, ex.INT_HI, torch.float32, dev, 7 * M + N1)
    bbuf = ex.rand_ints((M, N2 + 3), ex.INT_LO, ex.INT_HI, torch.float32, dev, 9 * M + N2)
    for strided in (False, True):
        a = abuf[:, 3:3 + N1] if strided else abuf[:, :N1].contiguous()
        b = bbuf[:, 1:1 + N2] if strided else bbuf[:, :N2].contiguous()
        ref = a.double().t() @ b.double()
        for acc in (False, True):
            what = "gemm_tn_f32 %s strided=%d accumulate=%d" % ((M, N1, N2), strided, acc)
            cols = N2 + (7 if strided else 0)
            buf = torch.full((N1 + GUARD, cols), SENTINEL, device=dev)
            out = buf[:N1, 2:2 + N2] if strided else buf[:N1]
            c0 = ex.rand_ints((N1, N2), ex.C0_LO, ex.C0_HI, torch.float32, dev, N1 + N2)
            if acc:
                out.copy_(c0)
            before = lib.dispatch_counts()
            lib.gemm_tn_f32(a, b, out, accumulate=acc)
            _ran(before, tn_f32=1)
            ex.assert_equal_everywhere(out.contiguous(), (ref + c0.double()).float() if acc else ref.float(), what)
            outside = torch.ones_like(buf, dtype=torch.bool)
            outside[:N1, 2:2 + N2] = False
            if not strided:
                outside[:N1] = False
            assert bool((buf[outside] == SENTINEL).all()), what + ": wrote outside the output view"


# ---- B. attention with closed forms ---------------------------------------------------------------------------------------------

@pytest.fixture(params=["coarse", "fine"])
def tile_rows(request, knobs):
    """128-row tiles or the 64-row tiles small launches take (as in tests/test_kernels_gpu.py)."""
    knobs.set("MRMT3_ATTN_FINE", "1" if request.param == "fine" else "0")
    return request.param


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _report(tag, devs):
    print("EXACT-B %-46s %s" % (tag, "  ".join("%s=%.3g" % kv for kv in devs.items())))


def _check_outputs(tag, c, got, H, names):
    """Every element of every tensor in `names` against the closed form; the message carries all measured deviations."""
    devs, errors = {}, []
    for n in names:
        want = getattr(c, n).to(got[n].device)
        try:
            if n == "lse":
                devs[n] = ex.check_lse("%s lse" % tag, got[n], want)
            else:
                devs[n] = ex.check_elements("%s %s" % (tag, n), got[n], want, ex.ATTN_TOL, H=H)
        except AssertionError as e:
            errors.append(str(e))
            devs[n] = ex.max_deviation(got[n], getattr(c, n))[0]
    _report(tag, devs)
    assert not errors, "%s: measured max deviations %s\n%s" % (tag, devs, "\n".join(errors))


def _bwd_modes(Lq, Lk, causal):
    modes = [("two-pass", 0)]
    if ex.onepass_takes(Lq, Lk, causal):
        modes.append(("one-pass", 1))
    return modes


def _run_mfma_attention(c, q, k, v, d_o, B, H, Lq, Lk, causal, knobs, tag, make_out=_nan_like):
    from mrmt3 import lib
    before = lib.dispatch_counts()
    o, lse, o_lo = lib.attn_fwd(q, k, v, B, H, Lq, Lk, causal, want_lo=True, out=make_out(q), out_lo=make_out(q))
    _ran(before, attn_fwd=1)
    _check_outputs(tag + " fwd", c, dict(o=o, lse=lse.double()), H, ("o", "lse"))
    for name, onepass in _bwd_modes(Lq, Lk, causal):
        knobs.set("MRMT3_ATTN_ONEPASS", onepass)
        knobs.set("MRMT3_ATTN_ONEPASS_MIN_BH", 1)
        dq, dk, dv = make_out(q), make_out(k), make_out(v)
        before = lib.dispatch_counts()
        lib.attn_bwd(q, k, v, o, d_o, lse, dq, dk, dv, B, H, Lq, Lk, causal, o_lo=o_lo)
        _ran(before, attn_bwd_onepass=onepass, attn_bwd=1 - onepass)
        _check_outputs("%s bwd %s" % (tag, name), c, dict(dq=dq, dk=dk, dv=dv), H, ("dq", "dk", "dv"))


@pytest.mark.parametrize("B,H,Lq,Lk,causal", ex.ATTN_SHAPES)
def test_attn_bf16_closed_form_every_element(dev, knobs, tile_rows, B, H, Lq, Lk, causal):
    c = ex.attention_case(B, H, Lq, Lk, causal)
    q, k, v, d_o = (getattr(c, n).to(dev).bfloat16() for n in ("q", "k", "v", "d_o"))
    _run_mfma_attention(c, q, k, v, d_o, B, H, Lq, Lk, causal, knobs, "mfma %s %s" % ((B, H, Lq, Lk, int(causal)), tile_rows))


def test_attn_bf16_closed_form_fused_qkv_layout(dev, knobs, tile_rows):
    """q, k, v (and dq, dk, dv) as column slices of one [rows, 1152] buffer."""
    B, H, L = 2, 6, 256
    c = ex.attention_case(B, H, L, L, False)
    qkv = torch.empty(B * L, 1152, device=dev, dtype=torch.bfloat16)
    for i, n in enumerate(("q", "k", "v")):
        qkv[:, 384 * i:384 * (i + 1)] = getattr(c, n).to(dev)
    grads = []

    def sliced(t):                                          # outputs: slices of NaN-filled fused buffers too
        grads.append(torch.full((B * L, 1152), float("nan"), device=dev, dtype=torch.bfloat16))
        return grads[-1][:, 384:768]

    _run_mfma_attention(c, qkv[:, :384], qkv[:, 384:768], qkv[:, 768:], c.d_o.to(dev).bfloat16(), B, H, L, L, False, knobs,
                        "mfma fused-qkv %s" % tile_rows, make_out=sliced)
    for g in grads:                                         # nothing outside the output's columns was written
        assert bool(torch.isnan(g[:, :384]).all()) and bool(torch.isnan(g[:, 768:]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,Lq,Lk,causal", [s for s in ex.ATTN_SHAPES if s[0] * s[1] <= 12])
def test_attn_general_kernels_closed_form_every_element(dev, dtype, B, H, Lq, Lk, causal):
    """attn_fwd_bias / attn_bwd_bias without a bias (f32 arithmetic on f32 or bf16 operands).  The 22 x 6 shape is the
    paired causal instantiation of the MFMA kernels; these kernels have one path for every batch size."""
    from mrmt3 import lib
    c = ex.attention_case(B, H, Lq, Lk, causal)
    q, k, v, d_o = (getattr(c, n).to(dev, dtype) for n in ("q", "k", "v", "d_o"))
    tag = "general %s %s" % ((B, H, Lq, Lk, int(causal)), str(dtype)[6:])
    before = lib.dispatch_counts()
    o, lse = lib.attn_fwd_bias(q, k, v, None, B, H, Lq, Lk, causal)
    _ran(before, attn_f32=1)
    _check_outputs(tag + " fwd", c, dict(o=o, lse=lse.double()), H, ("o", "lse"))
    before = lib.dispatch_counts()
    dq, dk, dv, dbias = lib.attn_bwd_bias(q, k, v, o, d_o, lse, None, B, H, Lq, Lk, causal)
    _ran(before, attn_f32=1)
    assert dbias is None
    _check_outputs(tag + " bwd", c, dict(dq=dq, dk=dk, dv=dv), H, ("dq", "dk", "dv"))


@pytest.mark.parametrize("site", ["self", "cross"])
def test_attn_varlen_closed_form_every_element(dev, site):
    """Packed rows of 0, 37, 300 and 1 tokens: causal self-attention over the packed keys, and cross-attention of every row
    to its own 320 dense keys.  The packed tail (Tcap - T rows of arbitrary q / k / v) must come back as zeros."""
    from mrmt3 import lib, packing
    H, L = 3, ex.VARLEN_L
    lengths = tuple(ex.VARLEN_LENGTHS)
    Bv, T = len(lengths), sum(lengths)
    cross = ex.VARLEN_CROSS_KEYS if site == "cross" else 0
    c = ex.varlen_case(lengths, H, cross)
    lab = np.full((Bv, L), -100, np.int64)
    for b, n in enumerate(lengths):
        lab[b, :n] = 5
    tcap = packing.capacity(packing.row_lengths(lab), Bv, L)
    pl = lib.pack_plan(torch.from_numpy(lab).to(dev), tcap, 0, 0)
    assert tcap > T and int(pl.err.item()) == 0
    g = torch.Generator().manual_seed(1)

    def padded(t, junk):                                    # [T, ...] -> [Tcap, ...]
        pad = torch.randint(-2, 3, (tcap - T, t.shape[1]), generator=g).float() if junk else torch.zeros(tcap - T, t.shape[1])
        return torch.cat([t, pad]).to(dev).bfloat16()

    q, d_o = padded(c.q, True), padded(c.d_o, False)
    k, v = (padded(c.k, True), padded(c.v, True)) if cross == 0 else (c.k.to(dev).bfloat16(), c.v.to(dev).bfloat16())
    want = ex.AttnCase()
    for n in ("o", "dq"):
        setattr(want, n, torch.cat([getattr(c, n), torch.zeros(tcap - T, H * 64)]))
    for n in ("dk", "dv"):
        setattr(want, n, torch.cat([getattr(c, n), torch.zeros(tcap - T, H * 64)]) if cross == 0 else getattr(c, n))
    want.lse = c.lse
    before = lib.dispatch_counts()
    o, lse, o_lo = lib.attn_fwd_varlen(q, k, v, pl, H, cross, cross == 0, want_lo=True)
    _ran(before, attn_fwd_varlen=1)
    tag = "varlen %s" % site
    _check_outputs(tag + " fwd", want, dict(o=o, lse=lse[:, :T].double()), H, ("o", "lse"))
    dq, dk, dv = _nan_like(q), _nan_like(k), _nan_like(v)
    before = lib.dispatch_counts()
    lib.attn_bwd_varlen(q, k, v, o, d_o, lse, dq, dk, dv, pl, H, cross, cross == 0, o_lo=o_lo)
    _ran(before, attn_bwd_varlen=1)
    _check_outputs(tag + " bwd", want, dict(dq=dq, dk=dk, dv=dv), H, ("dq", "dk", "dv"))


# ---- C. Gaussian inputs, a bound per row -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,Lq,Lk,causal", ex.ROW_BOUND_SHAPES)
def test_attn_bwd_bf16_gaussian_inputs_bounded_per_row(dev, knobs, B, H, Lq, Lk, causal):
    """For every 64-wide row r of O, dQ, dK, dV, per head: e_r = |got_r - ref_r| / max(|ref_r|, 1e-3 median row norm) against
    fp64 autograd on the inputs of test_attn_bwd_bf16; max_r e_r of the kernels is at most 4 x that of the fp64 restatement
    with the kernels' rounding points (P and dS to bf16 before their products, bf16 outputs).  The factor covers what the
    restatement leaves out: summation order, the exp2 and rcp approximations, delta from the hi/lo output."""
    from mrmt3 import lib
    q, k, v, d_o = ex.gaussian_attention_inputs(B, H, Lq, Lk, dev)
    ref = dict(zip(("o", "lse", "dq", "dk", "dv"), ex.attention_autograd(q, k, v, d_o, B, H, Lq, Lk, causal)))
    model = dict(zip(("o", "dq", "dk", "dv"), ex.attention_rounded(q, k, v, d_o, B, H, Lq, Lk, causal)))
    limit = {n: ex.ROW_BOUND_FACTOR * ex.row_errors(model[n], ref[n], H).max().item() for n in model}
    o, lse, o_lo = lib.attn_fwd(q, k, v, B, H, Lq, Lk, causal, want_lo=True)
    failures = []
    for name, onepass in _bwd_modes(Lq, Lk, causal):
        knobs.set("MRMT3_ATTN_ONEPASS", onepass)
        knobs.set("MRMT3_ATTN_ONEPASS_MIN_BH", 1)
        dq, dk, dv = _nan_like(q), _nan_like(k), _nan_like(v)
        before = lib.dispatch_counts()
        lib.attn_bwd(q, k, v, o, d_o, lse, dq, dk, dv, B, H, Lq, Lk, causal, o_lo=o_lo)
        _ran(before, attn_bwd_onepass=onepass, attn_bwd=1 - onepass)
        for n, got in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            e = ex.row_errors(got, ref[n], H)
            worst, at = e.max().item(), int(e.reshape(-1).argmax())
            ratio = worst / (limit[n] / ex.ROW_BOUND_FACTOR)
            print("EXACT-C %s %-8s %-2s max e_r kernel %.3e restatement %.3e ratio %.2f" % (
                (B, H, Lq, Lk, int(causal)), name, n, worst, limit[n] / ex.ROW_BOUND_FACTOR, ratio))
            if not worst <= limit[n]:
                failures.append("%s %s: max e_r %.3e at (row, head) = %s > %g x %.3e (ratio %.2f)" % (
                    name, n, worst, divmod(at, H), ex.ROW_BOUND_FACTOR, limit[n] / ex.ROW_BOUND_FACTOR, ratio))
    assert not failures, "\n".join(failures)
