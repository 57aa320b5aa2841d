"""Element-exact tests of the per-layer kernels of the KV-cached decode step (csrc/decode.hip) on a real MI355X: probe decoders.

A probe (tests/_exact_decode.py, proven on the CPU by tests/test_exact_decode_cpu.py) is a one-layer handle (H = 6, d_ff = 1024)
driven through the existing C ABI only: mrmt3_decoder_create / begin / set_prefix / run / logits.  Its inputs x0[b][t] are fed
as prefix rows with a zero position table, so no step depends on an emitted token and nothing carries over from step to step
but the K/V cache.  Weights, cross K|V and inputs are built so that the logits of every step show one kernel's output at every
element; every (row, step, element) is asserted, against a closed form or a float64 restatement with a derived bound.  No
assertion here is a norm, a median or a maximum over rows.

Handles: f32 with B = 3; bf16 with B = 3 and 8 (one weight row x one sequence per wave); bf16 with B = 9 and 17, and 256 where
noted (16 rows x 16 sequences on the matrix cores, partial and full tiles).  The matrix-core path is selected by
`bf16 && B > 8 && inner == 384 && d_ff == 1024` (`step()`, DEC_MFMA_ABOVE = 8) and no dispatch counter exists for it: the probes
rely on that rule, and a change of DEC_MFMA_ABOVE must revisit the batch sizes here.

Which probe reaches which kernel instance (every probe launches every kernel of the step; listed is where an instance's OUTPUT
is asserted per element):
  dec_norm_gemv<float, 1> / <bf16_t, 1>, dec_norm_gemm16<1>   q|k|v + cache append: probe 1, the self q probe
  dec_norm_gemv<float, 0> / <bf16_t, 0>, dec_norm_gemm16<0>   cross q (N = 384): probe 2, the cross q probe; lm_head (N = 1536,
                                                              1491, 512): probe 3, and the last kernel of every other probe
  dec_norm_gemv<float, 2> / <bf16_t, 2>, dec_norm_gemm16<2>   wi + gated GELU: probes 4 (res_ff) and 5
  dec_gemv_res<float, 1> / <bf16_t, 1>, dec_gemm16_res<3>     K = 384: probes 1, 2, the q probes (readout) and 4 (res_inner)
  dec_gemv_res<float, 2> / <bf16_t, 2>, dec_gemm16_res<8>     K = 1024: probes 4 (res_ff) and 5
  dec_attn<float> / dec_attn<bf16_t>                          len = t + 1 over the cache, 1..1024: probe 1; fixed length over
                                                              the caller's K|V (ld = 2 * inner, V at + inner), 1..2112: probe 2

Observed on an MI355X, largest error / derived bound over every element (`RATIO` lines; the bound comes from the operation
chain, never from these values):
                    f32-b3   bf16-b3  bf16-b8  bf16-b9  bf16-b17  bf16-b256
  lm_head V=1536    0.030    0 (bit-exact on every bf16 handle)
  lm_head V=1491    0.029    0
  res_inner         0.019    0.858    0.908    0.948    0.956
  res_ff            0.014    0.936    0.944    0.992    0.968
  geglu             0.027    0.984    0.989    0.993    0.994
  cross q           0.002    0.366    0.367    0.389    0.369
  self q            0.006    0.405    0.415    0.431    0.443
A bf16 handle's bound is, in all but the last two rows, the half ulp of the one bf16 rounding the final norm ends with (2^-8 of
the value, reached when the mantissa is near 1), which is why those figures sit just below 1: among ~10^5 elements one always
does.  It is still <= 1/4 of the smallest fault step of probe 4 (tests/test_exact_decode_cpu.py asserts that).
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_decode as ed  # noqa: E402

pytestmark = pytest.mark.gpu

# (id, bf16, B): the projections of the last two run on the matrix cores
HANDLES = [("f32-b3", False, 3), ("bf16-b3", True, 3), ("bf16-b8", True, 8), ("bf16-b9-mfma", True, 9),
           ("bf16-b17-mfma", True, 17)]
BIG = ("bf16-b256-mfma", True, 256)
LM_STEPS = 4
_ids = lambda hs: [h[0] for h in hs]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


def probe(kind, B, *args):
    """Built once and shared between the handles of one batch size, never modified (the 256-row probes are used once)."""
    return (_build if B == BIG[2] else _cached)(kind, B, *args)


def _build(kind, B, *args):
    p = {"self": ed.self_attention_probe, "cross": ed.cross_attention_probe, "q_cross": ed.q_cross_probe, "q_self": ed.q_self_probe,
         "lm_head": ed.lm_head_probe, "res_inner": ed.res_inner_probe, "res_ff": ed.res_ff_probe,
         "geglu": ed.geglu_probe}[kind](B, *args)
    ed.check_probe(p)
    return p


_cached = functools.lru_cache(maxsize=32)(_build)


def _report(what, ratio):
    print("RATIO %s %.3f" % (what, ratio))
    assert ratio <= 1.0


def run_probe(dev, p, bf16):
    """The probe through the C ABI on a stream of its own: one handle, one decoder_begin, x0 as the prefix, one replay and
    one copy of the logits per position.  -> logits [B, T, V] f32 on the host."""
    from mrmt3 import lib
    from mrmt3.decode import _Weights
    l = lib.load()
    dt = torch.bfloat16 if bf16 else torch.float32
    B, T, V, Lc = p.B, p.T, p.V, p.Lc
    max_len = T + 1                                          # set_prefix wants n_prefix < max_len
    on = lambda t, d: t.to(device=dev, dtype=d).contiguous()
    w = {k: on(t, torch.float32 if k.startswith("ln_") or k == "final_ln" else dt) for k, t in p.w.items()}
    embed = torch.zeros(1, ed.D, device=dev)
    pos = torch.zeros(max_len + 1, ed.D, device=dev)         # the tail reads row p + 1
    ckv = on(torch.cat([p.ck, p.cv], -1).view(1, B, Lc, 2 * ed.INNER), dt)
    x0 = on(p.x0, torch.float32)
    tokens = torch.zeros(B, max_len + 1, dtype=torch.int64, device=dev)
    out = torch.full((T, B, V), float("nan"), device=dev)
    keep = {k: (C.c_void_p * 1)(w[k].data_ptr()) for k in ("ln_self", "w_qkv", "w_o_self", "ln_cross", "w_q_cross", "w_o_cross",
                                                            "ln_ff", "w_wi", "w_wo")}
    ws = _Weights()
    ws.embed, ws.pos = embed.data_ptr(), pos.data_ptr()
    ws.lm_head, ws.final_ln = w["lm_head"].data_ptr(), w["final_ln"].data_ptr()
    for k, a in keep.items():
        setattr(ws, k, C.cast(a, C.POINTER(C.c_void_p)))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    h = C.c_void_p()
    lib._check(l.mrmt3_decoder_create(C.byref(h), 1, ed.D, ed.H, ed.DFF, V, B, max_len, Lc, lib.BF16 if bf16 else lib.F32,
                                      ed.EPS), "decoder_create")
    try:
        with torch.cuda.stream(stream):
            lib._check(l.mrmt3_decoder_begin(h, C.byref(ws), lib._p(ckv), B, Lc, lib._p(tokens), 0, 1, 0, lib._stream()),
                       "decoder_begin")
            lib._check(l.mrmt3_decoder_set_prefix(h, lib._p(x0), T, lib._stream()), "decoder_set_prefix")
            for t in range(T):
                lib._check(l.mrmt3_decoder_run(h, 1, lib._stream()), "decoder_run")
                lib._check(l.mrmt3_decoder_logits(h, lib._p(out[t]), B, lib._stream()), "decoder_logits")
        stream.synchronize()
        assert l.mrmt3_decoder_graph_captured(h) == 1
        assert l.mrmt3_decoder_capture_count(h) == 1
    finally:
        l.mrmt3_decoder_destroy(h)
    return out.transpose(0, 1).cpu()


# ---- 1. self-attention over the cache ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,bf16,B", HANDLES, ids=_ids(HANDLES))
def test_self_attention_over_the_cache_at_every_length(dev, tag, bf16, B):
    """len = 1..1024 in one run: every (step, row, head, dim) of o against the closed form."""
    p = probe("self", B, ed.SELF_LEN)
    ed.check("self", p, run_probe(dev, p, bf16), bf16, "self-attention " + tag)


# ---- 2. cross-attention ---------------------------------------------------------------------------------------------------------------

CROSS = [(h, Lc) for h in HANDLES for Lc in ed.ENC_LENS] + [(BIG, 257)]


@pytest.mark.parametrize("handle,Lc", CROSS, ids=["%s-enc%d" % (h[0], Lc) for h, Lc in CROSS])
def test_cross_attention_at_a_fixed_length(dev, handle, Lc):
    tag, bf16, B = handle
    p = probe("cross", B, ed.CROSS_STEPS, Lc)
    ed.check("cross", p, run_probe(dev, p, bf16), bf16, "cross-attention %s enc %d" % (tag, Lc))


@pytest.mark.parametrize("tag,bf16,B", HANDLES, ids=_ids(HANDLES))
def test_cross_q_projection_at_unsaturated_scores(dev, tag, bf16, B):
    p = probe("q_cross", B, ed.SHORT_STEPS)
    _report("q_cross " + tag, ed.check("q_cross", p, run_probe(dev, p, bf16), bf16, "cross q " + tag))


@pytest.mark.parametrize("tag,bf16,B", HANDLES, ids=_ids(HANDLES))
def test_self_q_projection_and_softmax_at_unsaturated_scores(dev, tag, bf16, B):
    p = probe("q_self", B, ed.SHORT_STEPS)
    _report("q_self " + tag, ed.check("q_self", p, run_probe(dev, p, bf16), bf16, "self q " + tag))


# ---- 3. lm_head -----------------------------------------------------------------------------------------------------------------------

LM = [(h, V) for h in HANDLES + [BIG] for V in ed.VOCABS]


@pytest.mark.parametrize("handle,V", LM, ids=["%s-v%d" % (h[0], V) for h, V in LM])
def test_lm_head_with_integer_operands(dev, handle, V):
    """bf16 handles: the float64 matmul bit for bit; f32 handles: within the bound of the operation chain."""
    tag, bf16, B = handle
    p = probe("lm_head", B, LM_STEPS, V)
    _report("lm_head %s V=%d" % (tag, V), ed.check("lm_head", p, run_probe(dev, p, bf16), bf16, "lm_head %s V=%d" % (tag, V)))


# ---- 4. residual projections ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,bf16,B", HANDLES, ids=_ids(HANDLES))
def test_res_inner_projection_on_an_exact_residual(dev, tag, bf16, B):
    p = probe("res_inner", B, ed.SHORT_STEPS, ed.RES_ENC_LEN)
    _report("res_inner " + tag, ed.check("res_inner", p, run_probe(dev, p, bf16), bf16, "res_inner " + tag))


@pytest.mark.parametrize("tag,bf16,B", HANDLES, ids=_ids(HANDLES))
def test_res_ff_projection_on_an_exact_residual(dev, tag, bf16, B):
    p = probe("res_ff", B, ed.SHORT_STEPS)
    _report("res_ff " + tag, ed.check("res_ff", p, run_probe(dev, p, bf16), bf16, "res_ff " + tag))


# ---- 5. gated GELU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,bf16,B", HANDLES, ids=_ids(HANDLES))
def test_gated_gelu_on_integer_gates(dev, tag, bf16, B):
    p = probe("geglu", B, ed.SHORT_STEPS)
    _report("geglu " + tag, ed.check("geglu", p, run_probe(dev, p, bf16), bf16, "geglu " + tag))
