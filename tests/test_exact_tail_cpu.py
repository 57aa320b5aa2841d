"""CPU proof of tests/_exact_tail.py, the tail probes of tests/test_exact_tail_gpu.py.

1. The construction conditions hold: every operand is a value bf16 holds, the residual that reaches the final norm is +-1 at all
   512 elements at every step, every partial sum of a logit stays below 2^24, the one softmax that is meant to saturate (the
   cross-attention over ONE key) is exactly 1, the finite logits are the closed form 2 (WE + WP + WR), no sampled u lies within
   SLACK of an interval edge, and every decision gap of a beam search is a designed tie or clears the score error.
2. The scenario ledgers are complete: the reference trace of every probe is scanned and every scenario the device tests are
   meant to exercise is reached, with the tied members placed as stated.
3. The checkers resolve the faults: the host emulation with one fault at a time fails the very checker the device tests use.
   The faults live in the emulation only; nothing injects one into a kernel or the library."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_tail as et  # noqa: E402
import sample_ref as sr  # noqa: E402
from beam_ref import BeamRef  # noqa: E402

ROWS = (3, 8, 9, 17)
VOCABS = (1536, 1491, 512, 65, 40, 2048)


def _as_device(tr):
    from types import SimpleNamespace
    return SimpleNamespace(tokens=tr.tokens, logp=tr.logp.float().double(), polls=tr.polls.int())


# ---- the greedy and sampled probes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VOCABS)
def test_greedy_probes_meet_the_construction_conditions(V):
    for B in (3, 17):
        for variant in ("open", "closed") + (("inf",) if V == 40 else ()):
            p = et.greedy_design(V, B, variant)
            tr = et.greedy_trace(p, et.greedy_ban(V))
            et.check_tail_probe(p)                                                       # any tokens
            et.check_tail_probe(p, torch.cat([torch.zeros(B, 1, dtype=torch.long), tr.tokens], 1))   # the decode's own


def test_the_256_row_probe_meets_the_construction_conditions():
    et.check_tail_probe(et.greedy_design(1536, 256, "closed"))


@pytest.mark.parametrize("V", VOCABS)
def test_greedy_ledger_is_complete(V):
    """Between the open and the closed probe of every (V, rows), without and with the ban (both bodies of dec_argmax see the
    same logits: LOGP does not change a token)."""
    for B in ROWS:
        for banned in (False, True):
            ban = et.greedy_ban(V) if banned else None
            seen, t0 = set(), time.time()
            for variant in ("open", "closed"):
                p = et.greedy_design(V, B, variant)
                seen |= et.greedy_ledger(p, et.greedy_trace(p, ban), ban)
            assert time.time() - t0 < 1.0
            assert et.greedy_required(V, B, banned) <= seen, (V, B, banned, et.greedy_required(V, B, banned) - seen)


def test_greedy_ledger_of_the_special_rows():
    p = et.greedy_design(40, 3, "inf")
    for ban in (None, et.greedy_ban(40)):
        tr = et.greedy_trace(p, ban)
        assert {"all-neginf", "tie:many", "fin:never"} <= et.greedy_ledger(p, tr, ban)
        assert bool(torch.isnan(tr.logp).all())                    # +inf next to -inf, or -inf alone: no distribution
    for V in (40, 65):
        p, ban = et.greedy_design(V, 3, "open"), np.ones(V, dtype=bool)
        tr = et.greedy_trace(p, ban)
        assert "all-banned" in et.greedy_ledger(p, tr, ban) and bool((tr.tokens == 0).all()) and bool(torch.isnan(tr.logp).all())


def test_greedy_ledger_of_256_rows():
    for variant, want in (("open", "fin:never"), ("closed", "fin:early")):
        p = et.greedy_design(1536, 256, variant)
        t0 = time.time()
        tr = et.greedy_trace(p)
        assert time.time() - t0 < 1.0
        assert {"fin:same-wg", "fin:diff-wg", want} <= et.greedy_ledger(p, tr)
    assert int(tr.polls[-1, 2]) < et.STEPS - 1 and len(set(tr.polls[:, 1].tolist())) == 2


def test_torch_argmax_is_the_documented_order():
    """torch.argmax (the reference) = the first NaN, else the first maximum (tests/sample_ref.py restates it in numpy)."""
    for V in (1491, 40):
        p = et.greedy_design(V, 9, "open")
        tr = et.greedy_trace(p)
        for t in range(et.STEPS):
            m = tr.logits[:, t].float()
            assert np.array_equal(torch.argmax(m, -1).numpy(), sr.torch_argmax(m.numpy()))


GREEDY_FAULTS = [("tie_high", True), ("nan_loses", False), ("nan_second", False), ("ban_after", True), ("col_v", False), ("no_pad", False),
                 ("pad_logp", False), ("fin_late", False)]


@pytest.mark.parametrize("fault,banned", GREEDY_FAULTS, ids=[f for f, _ in GREEDY_FAULTS])
@pytest.mark.parametrize("V", (1491, 40))
def test_greedy_checker_resolves(V, fault, banned):
    variant = "closed" if fault == "fin_late" else "open"
    p = et.greedy_design(V, 9, variant)
    ban = et.greedy_ban(V) if banned else None
    ref = et.greedy_trace(p, ban)
    et.check_greedy("emulation", _as_device(ref), ref)
    for logp in (True,) if fault == "pad_logp" else (True, False):
        with pytest.raises(AssertionError):
            et.check_greedy(fault, _as_device(et.greedy_trace(p, ban, fault=fault)), ref, logp)


def test_next_input_shows_in_the_next_logits():
    """A wrong embedded token moves the next step's designed logits at some element (WE differs between the classes)."""
    p = et.greedy_design(1491, 3, "open")
    a = et.design_logits(p, torch.tensor([5, 5, 5]), 3)
    b = et.design_logits(p, torch.tensor([5, 6, 5]), 3)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    rows = et.design_logits(p, torch.tensor([5, 5, 5]), 4)
    assert not torch.equal(rows[0], rows[1]) and not torch.equal(a[0], rows[0])      # the row and the position show too


@pytest.mark.parametrize("case", et.SAMPLED, ids=[c[0] for c in et.SAMPLED])
def test_sampled_cases_stay_clear_of_every_edge(case):
    tag, V, B, bf16, banned, top_k, seeds = case
    p = et.greedy_design(V, B, "open")
    ban = et.greedy_ban(V) if banned else None
    greedy = et.greedy_trace(p, ban)
    traces = []
    for seed in seeds:
        tr = et.greedy_trace(p, ban, (seed, 1.0, top_k, 1.0))
        drawn = np.isfinite(tr.edge)
        assert drawn.sum() >= 2 * B and float(tr.edge[drawn].min()) > 2 * sr.SLACK
        assert (tr.active.numpy() & ~drawn).any()                                # rows without a distribution: the greedy token
        assert not torch.equal(tr.tokens, greedy.tokens)
        et.check_greedy("emulation", _as_device(tr), tr)
        for fault in ("row_next", "step_next", "no_pad"):
            with pytest.raises(AssertionError):
                et.check_greedy(fault, _as_device(et.greedy_trace(p, ban, (seed, 1.0, top_k, 1.0), fault=fault)), tr, False)
        traces.append(tr)
    assert not torch.equal(traces[0].tokens, traces[1].tokens)


# ---- the beam probes ------------------------------------------------------------------------------------------------------------------

ALL_BEAM = et.BEAM + [et.BEAM_BIG]
_beam_ids = [c[0] for c in ALL_BEAM]
_events = {}


def _beam(case):
    p, ban = et.beam_case(case)
    t0 = time.time()
    ref = et.beam_trace(p, case[5], ban)
    took = time.time() - t0
    emu = et.beam_trace(p, case[5], ban, cls=et.BeamEmu, strict=None if case[7] else p)      # f32: duplicate rows alone may tie
    return p, ban, ref, emu, took


@pytest.mark.parametrize("case", ALL_BEAM, ids=_beam_ids)
def test_beam_probe_conditions_margins_and_emulation(case):
    tag, k, G, V, T, lp, kind, bf16, seed = case
    p, ban, ref, emu, took = _beam(case)
    assert took < 1.0
    et.check_tail_probe(p, torch.cat([torch.zeros(p.B, 1, dtype=torch.long), torch.from_numpy(np.stack(ref.tokens, 1))], 1))
    # the emulation that carries the ledger IS tests/beam_ref.py's search
    et.check_beam(tag, et.beam_as_device(emu, T + 1), ref, k)
    sc = np.stack(ref.scores)
    live = sc[np.isfinite(sc) & (np.abs(sc) < 1e8)]
    err = float(et.beam_tol(np.abs(live).max())) if len(live) else 0.0
    et.check_margins(tag, emu.ref.gaps, err)                 # ties in the three designed classes only; every other gap clears
    _events[tag] = emu.ref.events
    if not bf16:                                             # what an f32 handle keeps bit for bit
        assert not p.WR.any()
        assert len([g for g in et.identical_columns(p) if len(g) == 2]) >= 4


def test_beam_ledger_is_complete():
    for case in ALL_BEAM:
        if case[0] not in _events:
            _events[case[0]] = _beam(case)[3].ref.events
    seen = set().union(*_events.values())
    assert et.BEAM_SCENARIOS <= seen, et.BEAM_SCENARIOS - seen
    assert "group:done-while-others-run" in _events[et.BEAM_BIG[0]]
    for tag in ("k2-g3-v40-eos-only-bf16", "k2-g3-v40-eos-only-f32"):
        assert {"ban:fewer-than-2k-live", "ban:-inf-carried", "tie:-inf"} <= _events[tag]
    assert "nan:row" in _events["k2-g2-v40-nan-bf16"]


BEAM_FAULTS = {"rank_desc": "tie:", "eos_low": "eos:rank>=k-skipped", "drop_latest": "hyp:overflow-equal-lowest",
               "best_first": "end:equal-best", "done_gt": "done:at-equality"}
# Where the reference reaches the scenario and the fault still cannot be seen.  The hypothesis list is read once a step (and once
# after finalize): in these k = 8 cases the equal lowest entries all leave within one step's (or finalize's) several additions,
# so which of them left first leaves no trace.  The test asserts that these pass, so the list cannot grow unnoticed.
BEAM_UNSEEN = {("drop_latest", "k8-g2-v1536-bf16-mfma"), ("drop_latest", "k8-g1-v1491-ban-f32"), ("drop_latest", "k8-g1-v2048-bf16")}


@pytest.mark.parametrize("fault", sorted(BEAM_FAULTS))
def test_beam_checker_resolves(fault):
    """In EVERY case whose reference reaches the scenario a fault bends, the faulty emulation fails the checker, the cases of
    BEAM_UNSEEN excepted."""
    caught = []
    for case in et.BEAM:
        tag, k, G, V, T, lp, kind, bf16, seed = case
        p, ban, ref, emu, _ = _beam(case)
        if not any(e.startswith(BEAM_FAULTS[fault]) for e in emu.ref.events):
            continue
        bad = et.beam_as_device(et.beam_trace(p, lp, ban, cls=et.BeamEmu, fault=fault), T + 1)
        if (fault, tag) in BEAM_UNSEEN:
            et.check_beam(tag + " " + fault, bad, ref, k)
            continue
        with pytest.raises(AssertionError):
            et.check_beam(tag + " " + fault, bad, ref, k)
        caught.append(tag)
    assert caught, fault


def test_beam_ref_ranks_a_nan_first_and_is_unchanged_for_numbers():
    """tests/beam_ref.py gained the NaN rule (a NaN above every number, as torch.topk ranks it): for logits without a NaN its
    order is the old `lexsort((index, -score))`, and a NaN candidate now comes first."""
    rng = np.random.default_rng(5)
    flat = np.round(rng.standard_normal(500) * 2) / 2
    flat[rng.integers(0, 500, 40)] = -np.inf
    idx = np.arange(flat.size)
    assert np.array_equal(np.lexsort((idx, -flat, ~np.isnan(flat))), np.lexsort((idx, -flat)))
    for n in range(1, 9):                               # finalize's scan = the old stable sort + pop() on number lists
        h = [(float(v), i, i) for i, v in enumerate(rng.integers(0, 3, n))]
        b = 0
        for i in range(1, n):
            if h[i][0] >= h[b][0]:
                b = i
        assert h[b] == sorted(h, key=lambda e: e[0])[-1]
    ref = BeamRef(1, 2, 6)
    lg = np.zeros((2, 6))
    lg[0, 4] = np.nan
    par, tok, sc = ref.step(0, lg)
    assert par.tolist() == [0, 0] and tok.tolist() == [0, 2] and np.isnan(sc).all() and len(ref.hyps[0]) == 1


# ---- the reorder probes ----------------------------------------------------------------------------------------------------------------

_maps = {}


@pytest.mark.parametrize("case", et.REORDER, ids=[c[0] for c in et.REORDER])
def test_reorder_probe_conditions_emulation_and_margins(case):
    tag, k, G, read_layer, bf16, seed = case
    p = et.reorder_probe(k, G, read_layer, seed)
    et.check_reorder_probe(p)                    # bf16 operands, slots that tell rows apart, reads that cover positions and chunk edges
    t0 = time.time()
    logits = et.reorder_emulate(p, bf16)
    assert time.time() - t0 < 1.0
    ratio, tr = et.check_reorder(tag, p, logits, bf16)
    # the emulation IS the closed form (holders through the backpointers); what is left is the final norm's bf16 rounding of a
    # read-out value and of the pilot, half an ulp each: 2 x 2^-8 of a unit at most (layer 1's unit is 2.0 and cancels exactly)
    assert ratio <= (2 * 2.0 ** -8 / et.ed.ex.ATTN_TOL if bf16 and read_layer == 0 else 1e-6)
    emu = et.beam_trace(p, 1.0, p.ban, copy=logits, design=False, cls=et.BeamEmu)
    sc = np.stack(emu.scores)
    et.check_margins(tag, emu.ref.gaps, float(et.beam_tol(np.abs(sc[np.isfinite(sc)]).max())))
    assert not any(g[1] == 0 for g in emu.ref.gaps) and not any(emu.ref.done)     # nothing ties, no group ends: every step reorders
    _maps[tag] = et.reorder_ledger(p, tr)


def test_reorder_ledger_is_complete():
    for case in et.REORDER:
        if case[0] not in _maps:
            p = et.reorder_probe(*case[1:4], case[5])
            _maps[case[0]] = et.reorder_ledger(p, et.check_reorder(case[0], p, et.reorder_emulate(p, case[4]), case[4])[1])
    assert et.REORDER_MAPS <= set().union(*_maps.values())
    for case in et.REORDER:                      # what the device test of each case asserts it saw
        want = {"fan-out", "swap", "all-moved-k8"} if case[1] == 8 else {"fan-out", "swap", "identity", "3-cycle"}
        assert want <= _maps[case[0]], (case[0], want - _maps[case[0]])


def test_the_256_row_reorder_probes_meet_the_construction_conditions():
    for case in et.REORDER_BIG:
        et.check_reorder_probe(et.reorder_probe(*case[1:4], case[5]))


@pytest.mark.parametrize("fault", et.REORDER_FAULTS)
@pytest.mark.parametrize("case", [et.REORDER[0], et.REORDER[3], et.REORDER[4], et.REORDER[5]], ids=lambda c: c[0])
def test_reorder_checker_resolves(case, fault):
    """Every reorder fault, in the read layer's cache, fails the checker the device test uses.  Two cannot show where layer 0 is
    read: layer 1 on layer 0's previous parent map (layer 1 is not read there), and one slot from the sibling row (layer 0 is
    normed before the row bits arrive: the slot's row-bit elements are 0 in every row, its cache is unique per history only)."""
    tag, k, G, read_layer, bf16, seed = case
    if fault in ("layer1_prev_map", "slot_sibling") and read_layer == 0:
        return
    p = et.reorder_probe(k, G, read_layer, seed)
    with pytest.raises(AssertionError):
        et.check_reorder(tag + " " + fault, p, et.reorder_emulate(p, bf16, fault), bf16)
