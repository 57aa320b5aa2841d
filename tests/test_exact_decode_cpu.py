"""CPU proof of tests/_exact_decode.py, the probe decoders of tests/test_exact_decode_gpu.py.

1. The constructions are right: a plain-torch f32 emulation of the one-layer step (bf16 at the kernels' rounding points)
   passes every checker, the float64 restatement `oracle.t5_ref.decode_step_logits` (zero position table) agrees with the
   closed forms and with `_exact_decode.forward`, and every construction condition holds (margins, |x| <= 32, the cap on
   widened bounds, unsaturated gates on every wi row).
2. The checkers resolve the faults: the same emulation with one fault at a time fails the probe named for it.  The faults live
   in the emulation only; nothing injects one into a kernel or the library."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402
import _exact_decode as ed  # noqa: E402

BF16 = lambda t: t.float().bfloat16().double()
HANDLES = [pytest.param(True, id="bf16"), pytest.param(False, id="f32")]


@functools.lru_cache(maxsize=None)
def probe(kind, B, *args):
    p = {"self": ed.self_attention_probe, "cross": ed.cross_attention_probe, "lm_head": ed.lm_head_probe,
         "res_inner": ed.res_inner_probe, "q_cross": ed.q_cross_probe, "q_self": ed.q_self_probe, "res_ff": ed.res_ff_probe, "geglu": ed.geglu_probe}[kind](B, *args)
    ed.check_probe(p)
    return p


def _restated(p, bf16):
    from oracle import t5_ref
    sd, cfg = ed.state_dict(p)
    with torch.no_grad():
        return t5_ref.decode_step_logits(sd, cfg, torch.zeros(p.B, 0, dtype=torch.long), [p.ck], [p.cv], prefix=p.x0,
                                         rnd=BF16 if bf16 else None, pos=torch.zeros(p.T + 1, ed.D, dtype=torch.float64))


def _passes(kind, p, bf16):
    """The unmutated emulation passes, the restatement agrees with `forward` and passes too."""
    ratio = ed.check(kind, p, ed.emulate(p, bf16), bf16, "%s emulation" % kind)
    ref = _restated(p, bf16)
    fw = ed.reference(p, bf16)
    assert float((ref - fw.logits).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    if kind in ("self", "cross"):
        ed.check_attention(p, ref, "%s restatement" % kind)
    return ratio, fw


def _fails(kind, p, bf16, fault):
    with pytest.raises(AssertionError):
        ed.check(kind, p, ed.emulate(p, bf16, fault), bf16, "%s with %s" % (kind, fault))


# ---- the decode_step_logits argument ---------------------------------------------------------------------------------------------------

def test_pos_argument_defaults_to_the_sinusoid_table():
    from oracle import t5_ref
    p = probe("geglu", 2, 3)
    sd, cfg = ed.state_dict(p)
    ids = torch.zeros(p.B, 0, dtype=torch.long)
    a = t5_ref.decode_step_logits(sd, cfg, ids, [p.ck], [p.cv], prefix=p.x0)
    b = t5_ref.decode_step_logits(sd, cfg, ids, [p.ck], [p.cv], prefix=p.x0, pos=t5_ref.pos_emb(p.T, ed.D)[0])
    c = t5_ref.decode_step_logits(sd, cfg, ids, [p.ck], [p.cv], prefix=p.x0, pos=torch.zeros(p.T, ed.D))
    assert torch.equal(a, b) and not torch.equal(a, c)


# ---- 1. self-attention ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", HANDLES)
def test_self_attention_probe_at_the_device_shape(bf16):
    p = probe("self", 3, ed.SELF_LEN)
    assert p.margin >= ex.MIN_MARGIN
    assert set(p.o_want.unique().tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    _passes("self", p, bf16)
    # the rows' key sets differ, and the steps whose length is 1 mod 256 ask for the key just appended
    assert not torch.equal(p.o_want[0], p.o_want[1]) and not torch.equal(p.o_want[1], p.o_want[2])


SELF_FAULTS = ["drop_last_key", "ignore_512", "v_next", "other_head_k", "other_head_v", "swap_rows", "k_prev"] + \
              [("skip_kblock", "qkv", c) for c in range(0, ed.D, 32)] + [("skip_kblock", "o_self", c) for c in range(0, ed.INNER, 32)]


@pytest.mark.parametrize("fault", SELF_FAULTS, ids=str)
def test_self_attention_probe_resolves(fault):
    p = probe("self", 3, 600)                                # lengths 257 and 513, keys beyond 512
    if fault == SELF_FAULTS[0]:
        _passes("self", p, True)
    _fails("self", p, True, fault)
    if isinstance(fault, str):
        _fails("self", p, False, fault)


@pytest.mark.parametrize("proj", ["qkv", "o_self"])
def test_self_attention_probe_resolves_sequence_16_from_15(proj):
    p = probe("self", 17, 40)
    _passes("self", p, True)
    _fails("self", p, True, ("seq16", proj))


# ---- 2. cross-attention -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Lc", ed.ENC_LENS)
def test_cross_attention_probe_at_every_length(Lc):
    p = probe("cross", 3, ed.CROSS_STEPS, Lc)
    assert p.margin >= ex.MIN_MARGIN
    for bf16 in (True, False):
        _passes("cross", p, bf16)


CROSS_FAULTS = [("drop_last_key", 257), ("drop_last_key", 513), ("ignore_512", 513), ("ignore_512", 1001), ("v_next", 33),
                ("v_next", 257), ("other_head_k", 33), ("other_head_v", 33)] + \
               [(("skip_kblock", "o_cross", c), 33) for c in range(0, ed.INNER, 32)]


@pytest.mark.parametrize("fault,Lc", CROSS_FAULTS, ids=str)
def test_cross_attention_probe_resolves(fault, Lc):
    p = probe("cross", 3, ed.CROSS_STEPS, Lc)
    _fails("cross", p, True, fault)
    _fails("cross", p, False, fault)


@pytest.mark.parametrize("proj", ["q_cross", "o_cross"])
def test_cross_attention_probe_resolves_sequence_16_from_15(proj):
    p = probe("cross", 17, 8, 33)
    _passes("cross", p, True)
    _fails("cross", p, True, ("seq16", proj))


@pytest.mark.parametrize("bf16", HANDLES)
def test_q_cross_probe(bf16):
    """A saturated softmax forgives a query that lost a k-block (probe 2 passes with that fault); this probe does not."""
    sat = probe("cross", 3, ed.CROSS_STEPS, 33)
    ed.check("cross", sat, ed.emulate(sat, bf16, ("skip_kblock", "q_cross", 0)), bf16, "saturated")
    p = probe("q_cross", 17, ed.SHORT_STEPS)
    assert int((p.w["w_q_cross"] != 0).sum(0).min()) >= 2
    ratio, fw = _passes("q_cross", p, bf16)
    assert ratio <= 1
    assert float((fw.o_cross.abs() < 0.9).double().mean()) > 0.25          # the softmaxes are not saturated
    for fault in [("skip_kblock", "q_cross", c) for c in range(0, ed.D, 32)] + [("seq16", "q_cross"), "v_next", "other_head_k"]:
        _fails("q_cross", p, bf16, fault)


@pytest.mark.parametrize("bf16", HANDLES)
def test_q_self_probe(bf16):
    """The q rows of q|k|v alone: the saturated probe 1 forgives a lost k-block there, this probe does not."""
    q_only = ("skip_kblock", "qkv", 64, ed.INNER)
    sat = probe("self", 3, 40)
    ed.check("self", sat, ed.emulate(sat, bf16, q_only), bf16, "saturated")
    p = probe("q_self", 17, ed.SHORT_STEPS)
    ratio, fw = _passes("q_self", p, bf16)
    assert ratio <= 1
    assert float((fw.o_self.abs() < 0.9).double().mean()) > 0.25
    for fault in [("skip_kblock", "qkv", c, ed.INNER) for c in range(0, ed.D, 32)] + \
                 [("seq16", "qkv"), "v_next", "other_head_k", "other_head_v", "swap_rows", "k_prev"]:
        _fails("q_self", p, bf16, fault)


# ---- 3. lm_head -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", HANDLES)
@pytest.mark.parametrize("V", ed.VOCABS)
def test_lm_head_probe(V, bf16):
    p = probe("lm_head", 17, 4, V)
    ratio, fw = _passes("lm_head", p, bf16)
    assert ratio <= 1
    if bf16:
        assert torch.equal(fw.logits, p.want)                # the restatement is the integer matmul
    faults = [("skip_kblock", "lm_head", c) for c in range(0, ed.D, 32)] + [("seq16", "lm_head")]
    if V == 1491:
        faults += ["lm_last_twice", "lm_last_skipped"]
    for fault in faults:
        _fails("lm_head", p, bf16, fault)


# ---- 4. residual projections --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", HANDLES)
def test_res_inner_probe(bf16):
    p = probe("res_inner", 17, ed.SHORT_STEPS, ed.RES_ENC_LEN)
    assert float(p.x_want.abs().max()) <= ed.X_MAX
    assert int((p.w["w_o_cross"] != 0).sum(0).min()) >= 3    # every k covered by several rows
    ratio, fw = _passes("res_inner", p, bf16)
    assert ratio <= 1
    assert float((fw.x - p.x_want).abs().max()) <= (0 if bf16 else 1e-4)
    # the bound stays at <= 1/4 of the smallest fault step, (1/2) / rms, at every element of a bf16 handle
    assert bool((ed.res_inner_bound(p, fw, bf16) <= 1.001 * fw.rstd / 8).all())
    for fault in [("skip_kblock", "o_cross", c) for c in range(0, ed.INNER, 32)] + [("seq16", "o_cross"), "v_next"]:
        _fails("res_inner", p, bf16, fault)


@pytest.mark.parametrize("bf16", HANDLES)
def test_res_ff_probe(bf16):
    p = probe("res_ff", 17, ed.SHORT_STEPS)
    assert float(p.x_want.abs().max()) <= ed.X_MAX
    assert int((p.w["w_wo"] != 0).sum(0).min()) >= 2
    ratio, fw = _passes("res_ff", p, bf16)
    assert ratio <= 1
    assert float((fw.x - p.x_want).abs().max()) <= (1e-9 if bf16 else 1e-4)
    bound, share = ed.ffn_bound(p, fw, bf16)
    assert share == 0 and bool((bound <= 1.001 * fw.rstd / 8).all())
    for fault in [("skip_kblock", "wo", c) for c in range(0, ed.DFF, 32)] + [("seq16", "wo")]:
        _fails("res_ff", p, bf16, fault)


# ---- 5. gated GELU -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", HANDLES)
def test_geglu_probe(bf16):
    p = probe("geglu", 17, ed.SHORT_STEPS)
    ratio, fw = _passes("geglu", p, bf16)
    assert ratio <= 1
    h0, h1 = fw.h0.round(), fw.h1.round()
    assert float((fw.h0 - h0).abs().max()) <= (0 if bf16 else 1e-5) and float(h0.abs().max()) == 4 and float(h1.abs().max()) == 4
    _, share = ed.ffn_bound(p, fw, bf16)
    assert share <= ed.WIDE_CAP
    for fault in ["wi_pair", ("seq16", "wi"), ("seq16", "wo")] + [("skip_kblock", "wi", c) for c in range(0, ed.D, 32)] + \
                 [("skip_kblock", "wo", c) for c in range(0, ed.DFF, 32)]:
        _fails("geglu", p, bf16, fault)


@pytest.mark.parametrize("B", [3, 8, 9, 17, 256])
def test_every_wi_row_sees_unsaturated_gates(B):
    p = probe("geglu", B, ed.SHORT_STEPS)
    fw = ed.reference(p, True)
    live = (fw.h0.abs() <= 2) & (fw.h0 != 0) & (fw.h1 != 0)          # gelu_new far from both of its asymptotes, g nonzero
    assert bool(live.reshape(-1, ed.DFF).any(0).all())
    assert ed.ffn_bound(p, fw, True)[1] <= ed.WIDE_CAP


def test_a_widened_bound_is_counted():
    """The cap is not vacuous: a g placed next to a bf16 tie is found."""
    from types import SimpleNamespace
    h0 = torch.tensor([[[1.0, 2.0]]], dtype=torch.float64)
    g0 = ed.gelu_new(h0)
    a = g0.abs()
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    tie = (torch.floor(a / ulp) + 0.5) * ulp
    fw = SimpleNamespace(h0=h0, h1=torch.stack([tie[0, 0, 0] / g0[0, 0, 0], torch.tensor(1.0, dtype=torch.float64)]).view(1, 1, 2))
    dg, wide = ed.g_uncertainty(fw, True)
    assert wide.tolist() == [[[True, False]]] and float(dg[0, 0, 0]) >= float(ulp[0, 0, 0]) and float(dg[0, 0, 1]) == 0
