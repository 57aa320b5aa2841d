"""`scoring.build_problems` and the lists `scoring.pianoroll` launches with are, element for element, what they were before
the note-table path was folded together (entry expansion in `DeviceNotes.entries`, keys -> lists in `scoring._lists`, the
readback in `scoring._home`).  tests/golden/note_lists_parent.json holds every field of `Problems` for three family sets
and the arguments `pianoroll` hands to `lib.note_frames`, as plain lists, as the PARENT commit (named in the file) built
them on host tensors; the test rebuilds all of it and compares with `==`.

How the golden was recorded: the parent commit was checked out into a worktree of its own and `record()` of this module
was called with that tree (its root and its mr-mt3_amd/) on PYTHONPATH, so that `mrmt3`, `contrib` and `evaluate` were the
parent's; only this module and tests/_note_match.py came from here.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _note_match as M  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "note_lists_parent.json")
FAMILY_SETS = (None, ("on", "flat"), ("onoff", "on"))            # None: scoring.FAMILIES
ROLLS = (("all", None, None), ("by_program", None, "program"), ("empty_recording", 2, None))


def _pairs():
    """Six recording pairs: seeds 0..3 of the synthetic corpus, at position 2 a pair whose reference has no notes, and last
    a pair in which one side has an instrument without notes."""
    pairs = [M.synthetic_midi(seed, n=40) for seed in range(4)]
    pairs.insert(2, (M.midi([]), pairs[1][1]))
    pairs.append((M.midi([(5, False, []), (0, True, [(0.5, 0.6, 38)])]), pairs[0][1]))
    return pairs


def _plain(v):
    if isinstance(v, torch.Tensor):
        v = v.numpy()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, Exception):
        return [type(v).__name__, str(v)]
    if isinstance(v, (np.integer, np.floating, np.bool_)):
        return v.item()
    return v


class _Launched(Exception):
    pass


def _roll_arguments(scoring, notes, recording, by):
    """What `pianoroll` hands to `lib.note_frames`: the launch is replaced by a stub that keeps its arguments and raises."""
    from mrmt3 import lib
    seen = {}

    def stub(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first, fps, n_frames, with_roll=False):
        seen.update(idx=_plain(ref_idx), first=_plain(ref_first), fps=fps, n_frames=n_frames)
        raise _Launched()

    real, lib.note_frames = lib.note_frames, stub
    try:
        with pytest.raises(_Launched):
            scoring.pianoroll(notes, recording=recording, by=by)
    finally:
        lib.note_frames = real
    return seen


def build():
    """{name: value} of everything the golden holds, from the `mrmt3` package that is first on the path."""
    from mrmt3 import scoring
    from mrmt3.notes import DeviceNotes
    pairs = _pairs()
    ref = DeviceNotes.from_arrays([scoring.table_from_midi(r) for r, _ in pairs], "cpu")
    est = DeviceNotes.from_arrays([scoring.table_from_midi(e) for _, e in pairs], "cpu")
    out = {}
    for families in FAMILY_SETS:
        problems = scoring.build_problems(ref, est, *(() if families is None else (families,)))
        for field in dataclasses.fields(problems):
            out["problems[%s].%s" % ("all" if families is None else "+".join(families), field.name)] = _plain(
                getattr(problems, field.name))
    for name, recording, by in ROLLS:
        for k, v in _roll_arguments(scoring, ref, recording, by).items():
            out["pianoroll[%s].%s" % (name, k)] = v
    nothing = DeviceNotes.from_arrays([scoring.table_from_midi(M.midi([])) for _ in range(2)], "cpu")
    out["pianoroll[no_note_by_program]"] = _plain(scoring.pianoroll(nothing, by="program"))
    return out


def record(commit):
    with open(GOLDEN, "w") as f:
        json.dump({"parent": commit, "values": build()}, f, separators=(",", ":"))
        f.write("\n")


def test_problem_lists_and_roll_lists_are_the_parents():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["parent"]) == 40
    want, got = golden["values"], json.loads(json.dumps(build()))          # (tuples -> lists, as the golden's)
    compared = set()
    for name in want:
        assert name in got, name
        if got[name] != want[name]:
            if isinstance(want[name], list) and isinstance(got[name], list) and len(want[name]) == len(got[name]):
                at = next(i for i, (a, b) in enumerate(zip(got[name], want[name])) if a != b)
                pytest.fail("%s differs first at [%d]: %r, the parent's %r" % (name, at, got[name][at], want[name][at]))
            pytest.fail("%s: %r, the parent's %r" % (name, got[name], want[name]))
        compared.add(name)
    assert compared == set(want) == set(got)
    # the inputs are what the golden was meant to pin: all families, an empty pair, some hundreds of entries
    assert len(want["problems[all].pair"]) >= 50 and set(want["problems[all].family"]) == {0, 1, 2, 3, 4}
    assert len(want["problems[all].ref_idx"]) >= 500 and len(want["problems[all].est_idx"]) >= 500
    assert want["pianoroll[empty_recording].idx"] == [] and want["pianoroll[empty_recording].first"] == [0, 0]
    assert len(want["pianoroll[by_program].first"]) > len(want["pianoroll[all].first"]) == 7
    assert want["pianoroll[no_note_by_program]"] == [{}, {}]

