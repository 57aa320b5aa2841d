"""Packed decoder training, host side (mrmt3/packing.py, mrmt3/trainer.py): the plan the host computes from the labels, the
C ABI surface of the new entry points, and the variants that cannot be packed."""
import numpy as np
import pytest


def _restated(labels):
    """The plan restated with plain loops: len_b, offsets, granule, Tcap, dense fallback."""
    B, L = labels.shape
    lens = []
    for b in range(B):
        last = 0
        for t in range(L):
            if labels[b, t] != -100:
                last = t + 1
        lens.append(last)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G = max(256, ((B * L + 16 * 256 - 1) // (16 * 256)) * 256)
    T = int(off[-1])
    tcap = max(G, ((T + G - 1) // G) * G)
    tcap = min(tcap, B * L)
    return np.array(lens, np.int32), off, G, tcap


def _cases():
    from mrmt3.synthetic import synth_labels
    rs = np.random.RandomState(3)
    yield "slakh", synth_labels(64, 1024, full=False, seed=11)
    yield "full", synth_labels(8, 1024, full=True)
    yield "empty", np.full((4, 1024), -100, np.int64)
    yield "single", synth_labels(1, 1024, full=False, seed=5, mean_len=40)
    lab = rs.randint(3, 100, size=(5, 256)).astype(np.int64)
    lab[0] = -100                                   # an empty row
    lab[1, 17:] = -100
    lab[2, 3] = -100                                # an ignored label INSIDE the prefix does not end it
    lab[2, 200:] = -100
    yield "random", lab


@pytest.mark.parametrize("name,labels", list(_cases()), ids=[c[0] for c in _cases()])
def test_host_plan_matches_restatement(name, labels):
    from mrmt3 import packing
    B, L = labels.shape
    lens, off, G, tcap = _restated(labels)
    got = packing.row_lengths(labels)
    assert got.dtype == np.int32 and np.array_equal(got, lens)
    assert np.array_equal(np.concatenate([[0], np.cumsum(got)]), off)
    assert packing.granule(B, L) == G
    assert packing.capacity(got, B, L) == tcap
    assert tcap >= off[-1] and (tcap % G == 0 or tcap == B * L)
    if name == "full":
        assert tcap == B * L                        # nothing to save: the dense path
    if name == "empty":
        assert tcap == G                            # one granule of tail rows
    if name == "slakh":
        assert tcap < B * L // 2                    # mean 300 of 1024


def test_granule_gives_at_most_16_capacities():
    from mrmt3 import packing
    for B, L in ((64, 1024), (12, 1024), (2, 256), (3, 192), (1, 1024)):
        caps = {packing.capacity([T], B, L) for T in range(0, B * L + 1, 7)}
        assert len(caps) <= 16, (B, L, sorted(caps))


def test_new_symbols_in_header_and_signatures():
    from mrmt3 import lib
    names = {"mrmt3_pack_tile_entries", "mrmt3_pack_lengths", "mrmt3_pack_plan", "mrmt3_embed_fwd_packed",
             "mrmt3_attn_fwd_varlen", "mrmt3_attn_bwd_varlen"}
    assert names <= set(lib.header_symbols())
    assert names <= set(lib._SIGS)
    assert {"attn_fwd_varlen", "attn_bwd_varlen"} <= set(lib.COUNTER_NAMES)


def test_pack_targets_refused_for_segmem_v1():
    """Asked for packing, a segmem_v1 model (memory slots prepended to the decoder input) is refused at construction — before
    the trainer needs a device; other variants get past that check (and then need the GPU)."""
    from mrmt3.synthetic import T5_SMALL
    from mrmt3.trainer import Trainer
    from models.t5_segmem import T5SegMem
    from models.t5_segmem_v2 import T5SegMemV2
    with pytest.raises(ValueError, match="segmem_v1"):
        Trainer(T5SegMem(T5_SMALL, 1, 64), pack_targets=True)
    with pytest.raises(AssertionError, match="GPU"):
        Trainer(T5SegMemV2(T5_SMALL, 1, 64), pack_targets=True)
