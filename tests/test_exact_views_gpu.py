"""Element-exact GEMM tests on strided views inside wider buffers, on a real MI355X (constructions and checkers:
tests/_exact_views.py, proven on the CPU by tests/test_exact_views_cpu.py).

Every operand and every output is a view with columns to its left and right and rows above and below, the way the engine
hands column slices of `qkv`, `kv_all` and the transposed weights to the products.  Outside an operand view everything is
NaN: a result is right only if nothing outside the view reached any arithmetic.  Outside an output view everything is the
sentinel of tests/test_exact_gpu.py: a tile that stores past column N is seen as an overrun, not covered up by the next
row's own store.  The operand buffers must come back unchanged.

 a-f. gemm_nt (round-1 tile kernel, ping-pong kernel at both tile heights, split K), gemm_tn (tile kernel, tn8) and TnGroup
      on the small integers of tests/_exact.py: equal to the float64 product everywhere.
 g-i. the fused entry points (wi + GEGLU, projection + row kernels, lm_head + loss / log-probabilities): the same bits as the
      same call on contiguous copies of the same values — they are held to fp64 and to their two-kernel forms elsewhere; what
      is new here is the layout.
 Refusals: a stride that is no multiple of 16 bytes, a misaligned pointer, a stride smaller than the row — non-zero return
      code, no dispatch counter moves, the output is untouched.  Only what the argument checks refuse before any launch.

Comparisons are equality only, and every test asserts through the dispatch counters that the path it names ran.

Two cases are not what one would first write down, because the library refuses them on any layout, views or not:
  * a view with lda % 8 != 0 is outside mrmt3_gemm_rows_ok AND outside mrmt3_gemm_nt (rows must be 16-byte multiples), so the
    two-kernel form refuses it too: the test asserts both refusals;
  * V = 1491 (rows of f32 logits that are no multiple of 16 bytes) is refused by lm_head's product: the test asserts that the
    views and the contiguous copies are refused alike, before anything is written.

The whole file: 56 tests, 3.6 s on an MI355X (measured once)."""
import ctypes
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402
import _exact_views as xv  # noqa: E402
from test_exact_gpu import SENTINEL, _nt_raw, _ran  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
INVALID_ARG = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    t0 = time.time()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    print("EXACT-VIEWS wall time of this file: %.1f s" % (time.time() - t0))


def _pristine(*bufs):
    return [(b, b.clone()) for b in bufs]


# ---- a-c. gemm_nt ---------------------------------------------------------------------------------------------------------------

def _nt_views(M, N, K, dev, layout, what, expect, in_dtype=BF16, kinds=("f32", "bf16", "acc"), ws=None):
    """One NT product per output kind, every matrix a view: the exact result everywhere in the view, nothing written outside
    it, operands unchanged; `expect(kind)` are the counters one launch must move."""
    from mrmt3 import lib
    abuf, a = xv.operand((M, K), ex.INT_LO, ex.INT_HI, in_dtype, dev, 11 * M + K, *xv.margins(layout, "a", in_dtype))
    bbuf, b = xv.operand((N, K), ex.INT_LO, ex.INT_HI, in_dtype, dev, 13 * N + K, *xv.margins(layout, "b", in_dtype))
    c0 = ex.rand_ints((M, N), ex.C0_LO, ex.C0_HI, F32, dev, M + N)
    ref = a.double() @ b.double().t()                      # exact: integers far below 2^53
    assert float(ref.abs().max()) + 100 <= ex.int_sum_bound(K) < ex.EXACT_F32
    assert a.stride(0) != b.stride(0) or layout is xv.ENGINE
    keep = _pristine(abuf, bbuf)
    for kind in kinds:
        dt = BF16 if kind == "bf16" else F32
        cbuf, out = xv.output(M, N, dt, dev, SENTINEL, *xv.margins(layout, "c", dt), c0=c0 if kind == "acc" else None)
        before = lib.dispatch_counts()
        _nt_raw(a, b, out, kind == "acc", ws)
        _ran(before, **expect(kind))
        want = (ref + c0.double()).float() if kind == "acc" else ref.float()
        xv.check_product(cbuf, out, want.bfloat16() if kind == "bf16" else want, "%s %s" % (what, kind), SENTINEL, keep)


@pytest.mark.parametrize("M,N,K", xv.NT_TILE_SHAPES)
@pytest.mark.parametrize("in_dtype", [BF16, F32], ids=["bf16", "f32"])
def test_gemm_nt_tile_kernel_on_views(dev, in_dtype, M, N, K):
    """a. The round-1 tile kernel (M < 2048: gemm.hip launch_nt).  f32 operands have no bf16 output (gemm.hip refuses it)."""
    kinds = ("f32", "bf16", "acc") if in_dtype == BF16 else ("f32", "acc")
    _nt_views(M, N, K, dev, xv.RAGGED, "gemm_nt tile %s %s" % ((M, N, K), in_dtype), lambda kind: dict(gemm_nt_tile=1),
              in_dtype=in_dtype, kinds=kinds)


@pytest.mark.parametrize("M,N,K", xv.NT8_SMALL + xv.NT8_BIG)
def test_gemm_nt8_on_views(dev, knobs, M, N, K):
    """b. gemm_nt8_kernel, its f32, bf16 and accumulate instantiations at both tile heights, ragged M, shifted last tile."""
    knobs.set("MRMT3_GEMM8", 1)
    knobs.set("MRMT3_GEMM8_ALL", 1)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count & ~7
    small = -(-M // 256) * -(-N // 256) < cus              # gemm8.hip g8_plan
    assert small == ((M, N, K) in xv.NT8_SMALL), "the shape lists no longer reach both tile heights on %d CUs" % cus
    _nt_views(M, N, K, dev, xv.RAGGED, "gemm_nt8 %s" % ((M, N, K),), lambda kind: dict(gemm_nt8=1))


@pytest.mark.parametrize("M,N,K", xv.NT_ENGINE)
def test_gemm_nt_in_the_engine_layout(dev, knobs, M, N, K):
    """A and B as columns [384, 1152) of 1152-wide buffers, C as columns [768, 1536) of a 6144-wide one; the round-1 kernel
    below 2048 rows, the ping-pong kernel from there."""
    knobs.set("MRMT3_GEMM8", 1)
    knobs.set("MRMT3_GEMM8_ALL", 1)
    on8 = M >= 2048
    _nt_views(M, N, K, dev, xv.ENGINE, "gemm_nt engine layout %s" % ((M, N, K),),
              lambda kind: dict(gemm_nt8=int(on8), gemm_nt_tile=int(not on8)))


@pytest.mark.parametrize("M,N,K", xv.NT_SPLITK)
def test_gemm_nt_split_k_on_views(dev, M, N, K):
    """c. mrmt3_gemm_nt_ws split over K: the slab kernel reads strided A and B, the reduce writes strided C."""
    from mrmt3 import lib
    nbytes = int(lib.load().mrmt3_gemm_nt_workspace_bytes(M, N, K, 1))
    assert nbytes > 0, "not a split-K shape any more: pick one that is (csrc/gemm8.hip g8_splitk_plan)"
    if (M, N, K) == xv.NT_SPLITK[0]:                       # the smallest: one step down in any dimension does not split
        for m, n, k in ((M - 1, N, K), (M, N - 128, K), (M, N, K - 128)):
            assert int(lib.load().mrmt3_gemm_nt_workspace_bytes(m, n, k, 1)) == 0, (m, n, k)
    wbuf = torch.full((nbytes + 4 * 64,), 0x5A, device=dev, dtype=torch.uint8)
    _nt_views(M, N, K, dev, xv.RAGGED, "gemm_nt_ws split %s" % ((M, N, K),), lambda kind: dict(gemm_nt_splitk=1),
              ws=wbuf[:nbytes])
    assert bool((wbuf[nbytes:] == 0x5A).all()), "the split-K slab was overrun"


# ---- d-f. gemm_tn ---------------------------------------------------------------------------------------------------------------

def _tn_operands(M, N1, N2, dev, seed):
    abuf, a = xv.operand((M, N1), ex.INT_LO, ex.INT_HI, BF16, dev, 3 * M + N1 + seed, *xv.margins(xv.RAGGED, "a", BF16))
    bbuf, b = xv.operand((M, N2), ex.INT_LO, ex.INT_HI, BF16, dev, 5 * M + N2 + seed, *xv.margins(xv.RAGGED, "b", BF16))
    return abuf, a, bbuf, b


def _tn_views(M, N1, N2, dev, what, expect):
    from mrmt3 import lib
    abuf, a, bbuf, b = _tn_operands(M, N1, N2, dev, 0)
    c0 = ex.rand_ints((N1, N2), ex.C0_LO, ex.C0_HI, F32, dev, N1 + N2)
    ref = a.double().t() @ b.double()
    assert float(ref.abs().max()) + 100 <= ex.int_sum_bound(M) < ex.EXACT_F32
    keep = _pristine(abuf, bbuf)
    for acc in (False, True):
        cbuf, out = xv.output(N1, N2, F32, dev, SENTINEL, *xv.margins(xv.RAGGED, "c", F32), c0=c0 if acc else None)
        before = lib.dispatch_counts()
        lib.gemm_tn(a, b, out, accumulate=acc)
        _ran(before, **expect)
        xv.check_product(cbuf, out, (ref + c0.double()).float() if acc else ref.float(), "%s accumulate=%d" % (what, acc),
                         SENTINEL, keep)


@pytest.mark.parametrize("M,N1,N2", xv.TN_TILE_SHAPES)
def test_gemm_tn_tile_kernel_on_views(dev, knobs, M, N1, N2):
    """d. gemm_tn_kernel (MRMT3_TN8=0) and its slab reduce into a strided C."""
    knobs.set("MRMT3_TN8", 0)
    _tn_views(M, N1, N2, dev, "gemm_tn tile %s" % ((M, N1, N2),), dict(tn_tile=1))


@pytest.mark.parametrize("M,N1,N2", xv.TN8_SHAPES)
def test_gemm_tn8_on_views(dev, knobs, M, N1, N2):
    """e. gemm_tn8_kernel: ragged M read through the bounded buffer resource, with NaN rows right behind the view."""
    knobs.set("MRMT3_TN8", 1)
    knobs.set("MRMT3_TN8_ALL", 1)
    _tn_views(M, N1, N2, dev, "gemm_tn8 %s" % ((M, N1, N2),), dict(tn8=1))


def test_tn_group_on_views(dev):
    """f. One grouped launch; each site's A and B are column slices of ONE wider buffer (as the engine passes slices of qkv),
    each output a view, accumulate and overwrite mixed."""
    from mrmt3 import lib
    sites = []
    for i, (M, N1, N2) in enumerate(xv.TN_GROUP_SITES):
        la, gap, rb = 8, 16, 24                             # [NaN 8 | A N1 | NaN 16 | B N2 | NaN 24]
        buf = torch.full((xv.ABOVE + M + xv.BELOW, la + N1 + gap + N2 + rb), NAN, device=dev, dtype=BF16)
        a = buf[xv.ABOVE:xv.ABOVE + M, la:la + N1]
        b = buf[xv.ABOVE:xv.ABOVE + M, la + N1 + gap:la + N1 + gap + N2]
        a.copy_(ex.rand_ints((M, N1), ex.INT_LO, ex.INT_HI, BF16, dev, 100 + i))
        b.copy_(ex.rand_ints((M, N2), ex.INT_LO, ex.INT_HI, BF16, dev, 200 + i))
        acc = i % 2 == 0
        c0 = ex.rand_ints((N1, N2), ex.C0_LO, ex.C0_HI, F32, dev, 300 + i)
        cbuf, out = xv.output(N1, N2, F32, dev, SENTINEL, *xv.margins(xv.RAGGED, "c", F32), c0=c0 if acc else None)
        assert a.stride(0) == b.stride(0) == buf.shape[1] and lib.TnGroup.ok(a, b, out), (M, N1, N2)
        sites.append((a, b, buf, buf.clone(), cbuf, out, acc, c0))
    grp = lib.TnGroup()
    for a, b, _, _, _, out, acc, _ in sites:
        grp.add(a, b, out, accumulate=acc)
    before = lib.dispatch_counts()
    grp.flush()
    _ran(before, tn_group=1)
    for (M, N1, N2), (a, b, buf, keep, cbuf, out, acc, c0) in zip(xv.TN_GROUP_SITES, sites):
        ref = a.double().t() @ b.double()
        assert float(ref.abs().max()) + 100 <= ex.int_sum_bound(M) < ex.EXACT_F32
        xv.check_product(cbuf, out, (ref + c0.double()).float() if acc else ref.float(),
                         "TnGroup site %s accumulate=%d" % ((M, N1, N2), acc), SENTINEL, [(buf, keep)])


# ---- g. wi + GEGLU through the C ABI ---------------------------------------------------------------------------------------------

def _geglu_raw(x, wi, h, g, rows, dff, K, p):
    from mrmt3 import lib
    return lib.load().mrmt3_gemm_nt_geglu(lib._p(x), x.stride(0), lib._p(wi), wi.stride(0), lib._p(h), h.stride(0), lib._p(g),
                                          g.stride(0), rows, dff, K, p, 20240, None, 5, lib._stream())


# gemm8.hip mrmt3_gemm_nt_geglu: fused from rows >= MRMT3_GEGLU_FUSED_MIN_ROWS (2048) with dff % 128 == 0, K % 128 == 0, every
# stride a multiple of 8 and every pointer 16-byte aligned; below, mrmt3_gemm_nt (M < 2048: the tile kernel) + the row kernel
@pytest.mark.parametrize("rows,fused", [(2048, True), (2047, False)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_gemm_nt_geglu_on_views(dev, rows, fused, p):
    from mrmt3 import lib
    dff, K = 128, 128
    xbuf, x = xv.operand((rows, K), ex.INT_LO, ex.INT_HI, BF16, dev, 41, *xv.margins(xv.RAGGED, "a", BF16))
    wbuf, wi = xv.operand((2 * dff, K), ex.INT_LO, ex.INT_HI, BF16, dev, 42, *xv.margins(xv.RAGGED, "b", BF16))
    hbuf, h = xv.output(rows, 2 * dff, BF16, dev, SENTINEL, *xv.margins(xv.RAGGED, "c", BF16))
    gbuf, g = xv.output(rows, dff, BF16, dev, SENTINEL, 16, 8)
    keep = _pristine(xbuf, wbuf)
    expect = dict(gemm_nt_geglu=1) if fused else dict(gemm_nt_tile=1)
    before = lib.dispatch_counts()
    assert _geglu_raw(x, wi, h, g, rows, dff, K, p) == 0, lib.load().mrmt3_last_error()
    _ran(before, **expect)
    # the same call on contiguous copies
    xc, wc = x.contiguous(), wi.contiguous()
    hc, gc = torch.full((rows, 2 * dff), SENTINEL, device=dev, dtype=BF16), torch.full((rows, dff), SENTINEL, device=dev, dtype=BF16)
    before = lib.dispatch_counts()
    assert _geglu_raw(xc, wc, hc, gc, rows, dff, K, p) == 0, lib.load().mrmt3_last_error()
    _ran(before, **expect)
    ref = x.double() @ wi.double().t()
    assert float(ref.abs().max()) <= ex.int_sum_bound(K) < ex.EXACT_F32
    what = "gemm_nt_geglu rows=%d p=%g" % (rows, p)
    xv.check_product(hbuf, h, ref.float().bfloat16(), what + " h", SENTINEL, keep)
    xv.assert_same_bits(g.contiguous(), gc, what + " g")
    xv.assert_outside_untouched(gbuf, xv.box_of(gbuf, g), what + " g", SENTINEL)
    assert bool(torch.isfinite(gc.float()).all()) and bool((gc != SENTINEL).all()) and float(gc.float().abs().max()) > 0


# ---- h. projection + row kernels ---------------------------------------------------------------------------------------------------

def _gauss(shape, scale, seed, dev, dtype=BF16):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(dtype)


def _gauss_view(shape, scale, seed, dev, role):
    buf, v = xv.view_in(shape[0], shape[1], BF16, dev, NAN, *xv.margins(xv.RAGGED, role, BF16))
    v.copy_(_gauss(shape, scale, seed, dev))
    return buf, v


ROWS_SHAPES = [(40, 128), (1000, 384)]                     # (rows, K): one partial tile; ragged rows over several tiles


@pytest.fixture(params=[64, 128], ids=["tile64", "tile128"])
def rows_bm(request, knobs):
    knobs.set("MRMT3_ROWS_BM", request.param)              # gemm_rows.hip gr_bm: two instantiations
    return request.param


def _both_layouts(run, a_view, w_view, counter):
    """run(a, w) on the views and on contiguous copies; each launch moves `counter` by one and nothing else."""
    from mrmt3 import lib
    outs = []
    for a, w in ((a_view, w_view), (a_view.contiguous(), w_view.contiguous())):
        before = lib.dispatch_counts()
        outs.append(run(a, w))
        _ran(before, **{counter: 1})
    return outs


@pytest.mark.parametrize("rows,K", ROWS_SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gemm_nt_addnorm_on_views(dev, rows_bm, rows, K, p):
    from mrmt3 import lib
    abuf, a = _gauss_view((rows, K), 1.0, 1, dev, "a")
    wbuf, w = _gauss_view((512, K), K ** -0.5, 2, dev, "b")
    assert lib.gemm_rows_ok(a, w) and a.stride(0) > K and w.stride(0) > K
    x0, wn = _gauss((rows, 512), 1.0, 3, dev, F32), 1.0 + 0.1 * _gauss((512,), 1.0, 4, dev, F32)
    keep = _pristine(abuf, wbuf)
    run = lambda a_, w_: lib.gemm_nt_addnorm(a_, w_, x0, wn, 1e-6, p=p, seed=365, stream_y=11, stream_out=12)
    got, want = _both_layouts(run, a, w, "gemm_nt_addnorm")
    for name, g_, w_ in zip(("x1", "xn", "rstd"), got, want):
        xv.assert_same_bits(g_, w_, "gemm_nt_addnorm %s tile %d p=%g: %s" % ((rows, K), rows_bm, p, name))
        assert bool(torch.isfinite(g_.float()).all()), name
    for i, (buf, k) in enumerate(keep):
        xv.assert_same_bits(buf, k, "gemm_nt_addnorm: operand buffer %d was written" % i)


@pytest.mark.parametrize("rows,K", ROWS_SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gemm_nt_normbwd_on_views(dev, rows_bm, rows, K, p):
    from mrmt3 import lib
    abuf, a = _gauss_view((rows, K), 1.0, 11, dev, "a")
    wbuf, wt = _gauss_view((512, K), K ** -0.5, 12, dev, "b")
    assert lib.gemm_rows_ok(a, wt)
    dres, x1 = _gauss((rows, 512), 1.0, 13, dev), _gauss((rows, 512), 1.5, 14, dev, F32)
    rstd = torch.rsqrt((x1 * x1).mean(-1) + 1e-6)
    wn = 1.0 + 0.1 * _gauss((512,), 1.0, 15, dev, F32)
    keep = _pristine(abuf, wbuf)

    def run(a_, w_):
        dw = torch.zeros(512, device=dev)
        dx1, dy = lib.gemm_nt_normbwd(a_, w_, dres, x1, rstd, wn, dw, p=p, seed=99, stream_y=21)
        return dx1, dy, dw

    got, want = _both_layouts(run, a, wt, "gemm_nt_normbwd")
    for name, g_, w_ in zip(("dx1", "dy", "dw"), got, want):
        xv.assert_same_bits(g_, w_, "gemm_nt_normbwd %s tile %d p=%g: %s" % ((rows, K), rows_bm, p, name))
        assert bool(torch.isfinite(g_.float()).all()) and float(g_.float().abs().max()) > 0, name
    for i, (buf, k) in enumerate(keep):
        xv.assert_same_bits(buf, k, "gemm_nt_normbwd: operand buffer %d was written" % i)


@pytest.mark.parametrize("rows,K", ROWS_SHAPES)
@pytest.mark.parametrize("dff", [512, 1024])
def test_gemm_nt_geglubwd_on_views(dev, rows_bm, rows, K, dff):
    from mrmt3 import lib
    ybuf, dy = _gauss_view((rows, K), 1.0, 41, dev, "a")
    wbuf, wt = _gauss_view((dff, K), K ** -0.5, 42, dev, "b")
    assert lib.gemm_rows_ok(dy, wt, N=dff)
    h = _gauss((rows, 2 * dff), 1.0, 43, dev)
    keep = _pristine(ybuf, wbuf)
    run = lambda a_, w_: lib.gemm_nt_geglubwd(a_, w_, h, p=0.1, seed=7, stream_id=31)
    got, want = _both_layouts(run, dy, wt, "gemm_nt_geglubwd")
    xv.assert_same_bits(got, want, "gemm_nt_geglubwd %s dff=%d tile %d" % ((rows, K), dff, rows_bm))
    assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0
    for i, (buf, k) in enumerate(keep):
        xv.assert_same_bits(buf, k, "gemm_nt_geglubwd: operand buffer %d was written" % i)


def test_a_view_outside_gemm_rows_ok_is_refused_by_both_forms(dev):
    """lda % 8 != 0: rows that are no multiple of 16 bytes.  mrmt3_gemm_rows_ok says no, the fused entry point refuses — and so
    does mrmt3_gemm_nt, the first half of the two-kernel form (gemm.hip: row strides must be 16-byte multiples): there is no
    layout-tolerant fallback for such a view, the caller has to copy it.  Nothing is launched or written by either."""
    from mrmt3 import lib
    rows, K = 40, 128
    buf = _gauss((rows + 4, K + 12 + 32), 1.0, 5, dev)
    a = buf[:rows, 8:8 + K]                                 # 16-byte aligned start, lda = K + 44
    w = _gauss((512, K), K ** -0.5, 6, dev)
    assert a.stride(0) % 8 == 4 and a.data_ptr() % 16 == 0 and not lib.gemm_rows_ok(a, w) and lib.gemm_rows_ok(a.contiguous(), w)
    x0, wn = _gauss((rows, 512), 1.0, 7, dev, F32), torch.ones(512, device=dev)
    x1 = torch.full((rows, 512), SENTINEL, device=dev)
    before = lib.dispatch_counts()
    with pytest.raises(RuntimeError, match="gemm_nt_addnorm: unsupported shape"):
        lib.gemm_nt_addnorm(a, w, x0, wn, 1e-6, x1=x1)
    y = torch.full((rows, 512), SENTINEL, device=dev, dtype=BF16)
    with pytest.raises(RuntimeError, match="row strides must be 16-byte multiples"):
        lib.gemm_nt(a, w, out=y)
    _ran(before)
    torch.cuda.synchronize()
    assert bool((x1 == SENTINEL).all()) and bool((y == SENTINEL).all())


# ---- i. lm_head + loss, lm_head + log-probabilities ------------------------------------------------------------------------------

LM_ROWS, LM_D, LM_CHUNK = 300, 512, 128                    # three chunks: 128, 128, 44 rows


def _lmhead_inputs(V, dev):
    dbuf, dec = _gauss_view((LM_ROWS, LM_D), 1.0, 51, dev, "a")
    wbuf, w = _gauss_view((V, LM_D), 0.02, 52, dev, "b")
    g = torch.Generator(device=dev).manual_seed(53)
    tg = torch.randint(0, V, (LM_ROWS,), device=dev, generator=g)
    tg[::5] = -100
    return dbuf, dec, wbuf, w, tg


def _lmhead_ce_raw(dec, w, tg, V, dl):
    """mrmt3_lmhead_ce_fwd_bwd as lib.lmhead_cross_entropy calls it, returning (code, the loss DOUBLE)."""
    from mrmt3 import lib
    L = lib.load()
    acc = torch.zeros(2, device=dec.device, dtype=torch.float64)
    den = ctypes.c_void_p(acc.data_ptr() + 8)
    lib._check(L.mrmt3_ce_count(lib._p(tg), LM_ROWS, 0, 1135, 1262, den, lib._stream()), "ce_count")
    ws = lib.workspace(LM_CHUNK * V * 4, dec.device)
    rc = L.mrmt3_lmhead_ce_fwd_bwd(lib._p(dec), dec.stride(0), lib._p(w), w.stride(0), lib._p(tg), den, lib._p(acc), lib._p(dl),
                                   lib._dt(dl), LM_ROWS, V, LM_D, 0, 1135, 1262, 1.0, lib._p(ws), ws.numel(), LM_CHUNK,
                                   lib._stream())
    return rc, acc[:1].clone()


def _lmhead_logprob_raw(dec, w, tg, V, out):
    from mrmt3 import lib
    ws = lib.workspace(LM_CHUNK * V * 4, dec.device)
    return lib.load().mrmt3_lmhead_logprob(lib._p(dec), dec.stride(0), lib._p(w), w.stride(0), lib._p(tg), lib._p(out), LM_ROWS, V,
                                           LM_D, lib._dt(dec), lib._p(ws), ws.numel(), LM_CHUNK, lib._stream())


def test_lmhead_on_views(dev):
    """V = 1536.  The loss is compared as the double the kernel accumulates.  It is a sum of f32 values of 2^-6 and more (a
    row's NLL is within [4, 11] for these logits — asserted below — times 1 / 240, or f32 sums of such): each is a multiple of
    2^-29, the total stays below 2^4, so every partial sum in any order is exact in a double and the order in which the
    workgroups' atomic adds arrive cannot change a bit."""
    from mrmt3 import lib
    V = 1536
    dbuf, dec, wbuf, w, tg = _lmhead_inputs(V, dev)
    keep = _pristine(dbuf, wbuf)
    res = []
    for d_, w_ in ((dec, w), (dec.contiguous(), w.contiguous())):
        dl = torch.full((LM_ROWS, V), SENTINEL, device=dev, dtype=BF16)
        lp = torch.full((LM_ROWS,), SENTINEL, device=dev)
        before = lib.dispatch_counts()
        rc, loss = _lmhead_ce_raw(d_, w_, tg, V, dl)
        assert rc == 0, lib.load().mrmt3_last_error()
        _ran(before, gemm_nt_tile=3)                        # one product per chunk, M = 128, 128, 44
        before = lib.dispatch_counts()
        assert _lmhead_logprob_raw(d_, w_, tg, V, lp) == 0, lib.load().mrmt3_last_error()
        _ran(before, gemm_nt_tile=3)
        res.append((loss, dl, lp))
    (loss_v, dl_v, lp_v), (loss_c, dl_c, lp_c) = res
    nll = -lp_c[tg != -100]
    assert 4.0 <= float(nll.min()) and float(nll.max()) <= 11.0 and int((tg != -100).sum()) == 240
    xv.assert_same_bits(loss_v, loss_c, "lmhead_ce loss (double)")
    xv.assert_same_bits(dl_v, dl_c, "lmhead_ce dlogits")
    xv.assert_same_bits(lp_v, lp_c, "lmhead_logprob")
    assert bool(torch.isfinite(dl_c.float()).all()) and bool((dl_c != SENTINEL).all()) and bool((lp_c[tg == -100] == 0).all())
    assert float(loss_c) > 0
    for i, (buf, k) in enumerate(keep):
        xv.assert_same_bits(buf, k, "lmhead: operand buffer %d was written" % i)


def test_lmhead_with_the_codec_vocabulary_is_refused_alike_on_views(dev):
    """V = 1491: a row of f32 logits is 5964 bytes, no multiple of 16, and lm_head's product refuses it (gemm.hip: C rows must be
    16-byte aligned) — on views exactly as on contiguous operands, before anything is launched or written."""
    from mrmt3 import lib
    V = 1491
    dbuf, dec, wbuf, w, tg = _lmhead_inputs(V, dev)
    for d_, w_ in ((dec, w), (dec.contiguous(), w.contiguous())):
        dl = torch.full((LM_ROWS, V), SENTINEL, device=dev, dtype=BF16)
        lp = torch.full((LM_ROWS,), SENTINEL, device=dev)
        before = lib.dispatch_counts()
        rc, loss = _lmhead_ce_raw(d_, w_, tg, V, dl)
        assert rc == INVALID_ARG and b"C rows must be 16-byte aligned" in lib.load().mrmt3_last_error()
        assert _lmhead_logprob_raw(d_, w_, tg, V, lp) == INVALID_ARG
        _ran(before)
        torch.cuda.synchronize()
        assert float(loss) == 0.0 and bool((dl == SENTINEL).all()) and bool((lp == SENTINEL).all())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def _addr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def test_gemm_nt_refuses_bad_strides_and_pointers(dev):
    """gemm.hip mrmt3_gemm_nt's argument checks, with and without a workspace.  Every buffer is large enough for the layout
    the arguments describe."""
    from mrmt3 import lib
    L = lib.load()
    M, N, K = 1030, 384, 2048                               # a split-K shape, so that mrmt3_gemm_nt_ws's own gate is met as well
    a = torch.zeros(M + 4, K + 32, device=dev, dtype=BF16)
    b = torch.zeros(N + 4, K + 32, device=dev, dtype=BF16)
    nbytes = int(L.mrmt3_gemm_nt_workspace_bytes(M, N, K, 1))
    assert nbytes > 0
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    ok = dict(A=0, lda=K + 8, B=0, ldb=K + 16, C=0, ldc=N + 8)
    cases = {
        "lda not a multiple of 16 bytes": dict(lda=K + 4),
        "ldb not a multiple of 16 bytes": dict(ldb=K + 4),
        "ldc not a multiple of 16 bytes": dict(ldc=N + 2),
        "A 8 bytes off": dict(A=8),
        "B 8 bytes off": dict(B=8),
        "C 8 bytes off": dict(C=8),
        "lda < K": dict(lda=K - 8),
        "ldb < K": dict(ldb=K - 8),
        "ldc < N": dict(ldc=N - 8),
    }
    for out_dtype, code in ((F32, 0), (BF16, 1)):
        c = torch.full((M + 4, N + 32), SENTINEL, device=dev, dtype=out_dtype)
        for name, change in cases.items():
            if out_dtype == BF16 and name.startswith("ldc not"):
                change = dict(ldc=N + 4)
            g = dict(ok, **change)
            args = (_addr(a, g["A"]), g["lda"], _addr(b, g["B"]), g["ldb"], _addr(c, g["C"]), g["ldc"], M, N, K, 1, code, 0)
            before = lib.dispatch_counts()
            assert L.mrmt3_gemm_nt(*args, lib._stream()) == INVALID_ARG, name
            assert L.mrmt3_last_error().startswith(b"gemm_nt: "), name
            assert L.mrmt3_gemm_nt_ws(*args, lib._p(ws), ws.numel(), lib._stream()) == INVALID_ARG, name + " (with a workspace)"
            _ran(before)
        torch.cuda.synchronize()
        assert bool((c == SENTINEL).all()), "a refused gemm_nt wrote its output"


def test_gemm_tn_and_tn_group_refuse_bad_strides(dev):
    """gemm.hip mrmt3_gemm_tn (strides only: it has no pointer check to send a misaligned pointer against) and gemm_tn8.hip
    mrmt3_tn_group_ok / mrmt3_tn_group_plan."""
    from mrmt3 import lib
    L = lib.load()
    M, N1, N2 = 1100, 384, 320
    a = torch.zeros(M + 4, N1 + 32, device=dev, dtype=BF16)
    b = torch.zeros(M + 4, N2 + 32, device=dev, dtype=BF16)
    c = torch.full((N1 + 4, N2 + 32), SENTINEL, device=dev)
    ws = lib.workspace(int(L.mrmt3_gemm_tn_workspace_bytes(M, N1, N2)), dev)
    ok = dict(lda=N1 + 8, ldb=N2 + 16, ldc=N2 + 4)
    for name, change in {"lda % 8": dict(lda=N1 + 4), "ldb % 8": dict(ldb=N2 + 4), "ldc % 4": dict(ldc=N2 + 2),
                         "lda < N1": dict(lda=N1 - 8), "ldb < N2": dict(ldb=N2 - 8), "ldc < N2": dict(ldc=N2 - 4)}.items():
        g = dict(ok, **change)
        before = lib.dispatch_counts()
        rc = L.mrmt3_gemm_tn(lib._p(a), g["lda"], lib._p(b), g["ldb"], lib._p(c), g["ldc"], M, N1, N2, 0, lib._p(ws), ws.numel(),
                             lib._stream())
        assert rc == INVALID_ARG and L.mrmt3_last_error().startswith(b"gemm_tn: "), name
        _ran(before)
    # the grouped launch: a site whose A rows are no multiple of 16 bytes is outside mrmt3_tn_group_ok, and the planner
    # refuses the whole group before anything is launched
    av, bv, cv = a[:M, 8:].as_strided((M, N1), (N1 + 12, 1)), b[:M, :N2], c[:N1, :N2]
    assert av.stride(0) % 8 == 4 and av.data_ptr() % 16 == 0 and not lib.TnGroup.ok(av, bv, cv) and lib.TnGroup.ok(a[:M, :N1], bv, cv)
    grp = lib.TnGroup()
    grp.add(av, bv, cv, accumulate=False)
    before = lib.dispatch_counts()
    with pytest.raises(RuntimeError, match="outside the grouped kernel's shapes"):
        grp.flush()
    _ran(before)
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all()), "a refused gemm_tn wrote its output"


def test_gemm_nt_geglu_refuses_rows_narrower_than_the_output(dev):
    """gemm8.hip mrmt3_gemm_nt_geglu: ldh < 2 dff, ldg < dff (both paths), and on the unfused path a g whose rows are no
    multiple of 16 bytes — refused before the product is launched, so that h is not written either."""
    from mrmt3 import lib
    L = lib.load()
    dff, K = 128, 128
    for rows in (2048, 2047):
        x = torch.zeros(rows, K, device=dev, dtype=BF16)
        wi = torch.zeros(2 * dff, K, device=dev, dtype=BF16)
        h = torch.full((rows + 4, 2 * dff + 32), SENTINEL, device=dev, dtype=BF16)
        g = torch.full((rows + 4, dff + 32), SENTINEL, device=dev, dtype=BF16)
        cases = [("ldh < 2 dff", 2 * dff - 8, dff + 8), ("ldg < dff", 2 * dff + 8, dff - 8)]
        if rows < 2048:
            cases.append(("ldg % 8 on the unfused path", 2 * dff + 8, dff + 4))
        for name, ldh, ldg in cases:
            before = lib.dispatch_counts()
            rc = L.mrmt3_gemm_nt_geglu(lib._p(x), K, lib._p(wi), K, lib._p(h), ldh, lib._p(g), ldg, rows, dff, K, 0.0, 1, None, 0,
                                       lib._stream())
            assert rc == INVALID_ARG and L.mrmt3_last_error().startswith(b"gemm_nt_geglu: "), (rows, name)
            _ran(before)
        torch.cuda.synchronize()
        assert bool((h == SENTINEL).all()) and bool((g == SENTINEL).all()), rows
