"""Constructions and checkers of the strided-view GEMM tests (tests/test_exact_views_gpu.py; proven on the CPU by
tests/test_exact_views_cpu.py).  Plain torch on whatever device the tensors live on; nothing here touches the library.

Every operand and every output of a product is a VIEW inside a wider, taller buffer, as the engine passes column slices of
`qkv`, `kv_all` and the transposed weights:
  * inside an operand view: the small integers of tests/_exact.py, so the result is the float64 product bit for bit;
  * outside an operand view: NaN.  A result can be right only if nothing outside the view reached any arithmetic — a value
    read and multiplied by zero still shows;
  * outside an output view: a sentinel no result equals, left and right of every row and in the rows above and below.  A
    tile that stores past column N lands in the columns to the right, not in the next row's own columns where that row's
    store would cover it up.
`emulate_nt` / `emulate_tn` restate a kernel on flat memory (pointer, row stride), with the addressing faults the checkers
must catch.
"""
import collections

import torch

import _exact as ex

ABOVE, BELOW = 2, 3                      # rows of the buffer above and below every view

# Margins left and right of a view in units of 16 bytes (8 bf16 or 4 f32 elements: every kernel's alignment rule).  Unequal,
# different for A, B and C (so that swapped strides differ), and no multiple of a 128-, 256- or 512-wide tile.
RAGGED = dict(a=(1, 3), b=(3, 2), c=(1, 3))
# The engine's own layout, in elements: an operand is columns [384, 1152) of a 1152-wide buffer (k | v of the fused qkv,
# WT[:, inner:]), an output columns [768, 1536) of a 6144-wide one (one layer's slice of kv_all).  Width 768 both ways.
ENGINE_W = 768
ENGINE = dict(a=(384, 0), b=(384, 0), c=(768, 6144 - 1536))

# ---- shapes, with the dispatcher's condition that puts them where they are (256 CUs) ------------------------------------------
NT_TILE_SHAPES = [(129, 136, 96), (1, 8, 32)]              # gemm.hip launch_nt: M < 2048, so not the ping-pong kernel
# gemm8.hip mrmt3_gemm_nt8_try with MRMT3_GEMM8_ALL=1: M >= 2048, N >= 256, N % 128 == 0, K % 128 == 0.  g8_plan: 128-row
# tiles (`small`) while ceil(M / 256) * ceil(N / 256) < 256 CUs, else 256-row tiles.  N = 384 and 1152: a shifted last tile.
NT8_SMALL = [(2049, 384, 128), (2049, 1152, 128), (2049, 512, 128), (2049, 384, 384), (2049, 1152, 384), (2049, 512, 384)]
NT8_BIG = [(13060, 1152, 128), (13060, 1152, 256), (32520, 384, 128), (32520, 512, 256)]     # 52 x 5, 128 x 2 tiles >= 256
# gemm8.hip g8_splitk_plan: M >= 1024, N >= 256, N % 128 == 0, K >= 2048, K % 128 == 0, ceil(M / 128) * ceil(N / 256) * 2 <= CUs,
# K / split >= 512.  (1024, 256, 2048) is the smallest; the second has a ragged M (mpad > M) and a shifted last tile.
NT_SPLITK = [(1024, 256, 2048), (1030, 384, 2048)]
NT_ENGINE = [(300, ENGINE_W, ENGINE_W), (2100, ENGINE_W, ENGINE_W)]       # round-1 kernel; ping-pong kernel (M >= 2048)
TN_TILE_SHAPES = [(64, 72, 40), (1000, 512, 384)]          # gemm.hip tn_plan with MRMT3_TN8=0
TN8_SHAPES = [(8200, 896, 320)]                            # gemm_tn8.hip mrmt3_tn8_plan with MRMT3_TN8_ALL=1: M >= 8192, N1 % 128 == 0, N2 % 64 == 0
TN_GROUP_SITES = ex.TN_GROUP_SITES                         # gemm_tn8.hip mrmt3_tn_group_ok: M >= 1024, N1 % 128 == 0, N2 % 64 == 0


def unit(dtype):
    """Elements in 16 bytes."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def margins(layout, role, dtype):
    """(left, right) in elements of `dtype` for role 'a', 'b' or 'c'."""
    l, r = layout[role]
    return (l, r) if layout is ENGINE else (l * unit(dtype), r * unit(dtype))


Box = collections.namedtuple("Box", "above left rows cols")


def view_in(rows, cols, dtype, device, fill, left, right, above=ABOVE, below=BELOW):
    """(buffer, view): buffer [above + rows + below, left + cols + right] filled with `fill`, view = buffer[above:above + rows,
    left:left + cols].  The view starts on a 16-byte boundary and its row stride is a multiple of 16 bytes."""
    u = unit(dtype)
    assert left % u == 0 and right % u == 0 and cols % u == 0, (left, right, cols, dtype)
    buf = torch.full((above + rows + below, left + cols + right), fill, dtype=dtype, device=device)
    return buf, buf[above:above + rows, left:left + cols]


def box_of(buf, view):
    off = view.storage_offset() - buf.storage_offset()
    return Box(off // buf.stride(0), off % buf.stride(0), view.shape[0], view.shape[1])


def operand(shape, lo, hi, dtype, device, seed, left, right):
    """Integers in lo..hi inside the view, NaN everywhere else in the buffer."""
    buf, view = view_in(shape[0], shape[1], dtype, device, float("nan"), left, right)
    view.copy_(ex.rand_ints(shape, lo, hi, dtype, device, seed))
    return buf, view


def output(rows, cols, dtype, device, fill, left, right, c0=None):
    """The sentinel everywhere; the view holds the integer start of an accumulate case when `c0` is given."""
    buf, view = view_in(rows, cols, dtype, device, fill, left, right)
    if c0 is not None:
        view.copy_(c0)
    return buf, view


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_outside_untouched(buffer, view_box, what, fill):
    """Every element of `buffer` outside `view_box` still has the bit pattern of `fill` (NaN included); names the first changed
    element by (row, column) relative to the view."""
    want = torch.full_like(buffer, fill)
    b = Box(*view_box)
    inside = torch.zeros(buffer.shape, dtype=torch.bool, device=buffer.device)
    inside[b.above:b.above + b.rows, b.left:b.left + b.cols] = True
    bad = (_bits(buffer) != _bits(want)) & ~inside
    if bool(bad.any()):
        idx = bad.nonzero()
        r, c = idx[0].tolist()
        raise AssertionError("%s: %d elements outside the view were written; the first at (row, column) = (%d, %d) relative to "
                             "the [%d, %d] view holds %r" % (what, idx.shape[0], r - b.above, c - b.left, b.rows, b.cols,
                                                             float(buffer[r, c])))


def assert_same_bits(got, want, what):
    """Bit patterns equal everywhere (NaN = the same NaN), with the first differing index in the message."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if bool(bad.any()):
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError("%s: %d of %d elements differ in bits; the first at %s: got %r, want %r" % (
            what, idx.shape[0], got.numel(), i, float(got[i]), float(want[i])))


def check_product(out_buf, out_view, want, what, fill, operands=()):
    """The three checks of one product: the view equals `want` everywhere, nothing outside it was written, and no operand
    buffer (`operands`: (buffer, pristine copy) pairs) changed.  All three run; the message carries every failure."""
    checks = [lambda: ex.assert_equal_everywhere(out_view.contiguous(), want, what),
              lambda: assert_outside_untouched(out_buf, box_of(out_buf, out_view), what, fill)]
    for i, (buf, keep) in enumerate(operands):
        checks.append(lambda i=i, buf=buf, keep=keep: assert_same_bits(buf, keep, "%s: operand buffer %d was written" % (what, i)))
    errors = []
    for check in checks:
        try:
            check()
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, "\n".join(errors)


# ---- a kernel restated on flat memory -------------------------------------------------------------------------------------------

class Mem:
    """What a kernel is handed for one matrix: the buffer's flat storage, the element offset of the view's first element, the
    row stride."""

    def __init__(self, buf, view):
        self.flat = buf.reshape(-1)
        assert self.flat.data_ptr() == buf.data_ptr()           # shares the buffer's storage: stores are seen by the checks
        self.base = view.storage_offset() - buf.storage_offset()
        self.ld = buf.stride(0)

    def index(self, rows, cols, base=None, ld=None):
        """Flat indices of rows x cols (1-D index tensors), clipped into the storage (a real kernel would fault)."""
        base = self.base if base is None else base
        ld = self.ld if ld is None else ld
        i = base + rows[:, None] * ld + cols[None, :]
        return i.clamp_(0, self.flat.numel() - 1)

    def load(self, rows, cols, **kw):
        return self.flat[self.index(rows, cols, **kw)].double()

    def store(self, rows, cols, values, **kw):
        i = self.index(rows, cols, **kw)
        self.flat[i.reshape(-1)] = values.to(self.flat.dtype).reshape(-1)


FAULTS = ("base_dropped", "ld_is_width", "ld_swapped", "tile_past_n", "row_past_m", "zero_times_outside", "wrong_ldc")
TILE_N = 128                             # column tile of the emulated kernels


def _emulate(A, B, C, rows_a, cols_a, rows_b, cols_b, m, n, transposed, accumulate, fault):
    """C[m, n] (+)= A . B^T (NT: A [m, k], B [n, k]) or A^T . B (TN: A [k, m], B [k, n]); `fault` is one of FAULTS or None."""
    dev = A.flat.device
    ar = lambda x: torch.arange(x, device=dev)
    ka, kb = {}, {}
    if fault == "base_dropped":
        ka = dict(base=0)                                                   # reads from column 0 of the buffer
    elif fault == "ld_is_width":
        ka, kb = dict(ld=cols_a), dict(ld=cols_b)
    elif fault == "ld_swapped":
        ka, kb = dict(ld=B.ld), dict(ld=A.ld)
    a = A.load(ar(rows_a), ar(cols_a), **ka)
    b = B.load(ar(rows_b), ar(cols_b), **kb)
    acc = a.t() @ b if transposed else a @ b.t()
    if fault == "zero_times_outside":                                       # one element right of A's view, times zero
        acc[0, 0] += A.load(ar(1), torch.tensor([cols_a], device=dev))[0, 0] * 0.0
    if accumulate:
        acc = acc + C.load(ar(m), ar(n), **(dict(ld=n) if fault == "wrong_ldc" else {}))
    out_rows = ar(m + 1) if fault == "row_past_m" else ar(m)
    if fault == "row_past_m":
        acc = torch.cat([acc, acc[-1:]])
    for n0 in range(0, n, TILE_N):                                          # column tiles, the last one ragged
        w = TILE_N if fault == "tile_past_n" else min(TILE_N, n - n0)
        tile = torch.zeros(acc.shape[0], w, dtype=torch.float64, device=dev)
        keep = min(w, n - n0)
        tile[:, :keep] = acc[:, n0:n0 + keep]
        C.store(out_rows, n0 + ar(w), tile)


def emulate_nt(A, B, C, M, N, K, accumulate=False, fault=None):
    _emulate(A, B, C, M, K, N, K, M, N, False, accumulate, fault)


def emulate_tn(A, B, C, M, N1, N2, accumulate=False, fault=None):
    _emulate(A, B, C, M, N1, M, N2, N1, N2, True, accumulate, fault)
