"""`evaluate` — multi-track transcription scores for the MIDI files `test.py` writes, the build's
counterpart of the reference's evaluate.py:16-330 without pretty_midi / note_seq / mir_eval / librosa:
MIDI files are read by `contrib.midi_io.read_midi` (pretty_midi's conventions), note matching is
`contrib.transcription_metrics` (mir_eval's algorithm).  Function names, arguments and result keys are
the reference's.  CPU, host-side by default: nothing here touches the GPU path unless a `device` is named, and then only
the matching moves (`mrmt3.scoring`): the files are read and the results assembled by the same code.
"""
from __future__ import annotations

import collections
import concurrent.futures
import glob

import numpy as np

from contrib import midi_io
from contrib import transcription_metrics as tm


def get_granular_program(program_number, is_drum, granularity_type):
    """evaluate.py:16-22 ('flat': pitched vs drums; 'midi_class': the General-MIDI family of 8)."""
    if granularity_type == "full":
        return program_number
    if granularity_type == "midi_class":
        return (program_number // 8) * 8
    if granularity_type == "flat":
        return 0 if not is_drum else 1
    return None


def _midi(x):
    return x if isinstance(x, midi_io.MidiData) else midi_io.read_midi(x)


def transcription_metrics_result(n_ref, n_est, onoff, on):
    """The dict of `compute_transcription_metrics` from the two (precision, recall, f1, overlap) tuples."""
    keys = ("precision", "recall", "f1", "overlap")
    out = {"len_ref_intervals": n_ref, "len_est_intervals": n_est}
    out.update({f"onoff_{k}": v for k, v in zip(keys, onoff)})
    out.update({f"on_{k}": v for k, v in zip(keys, on)})
    return out


def program_aware_result(onset, groups, granularity_type):
    """The dict of `mt3_program_aware_note_scores`: `onset` the instrument-agnostic (precision, recall, f1), `groups` one
    ((program, is_drum), (precision, recall, f1), n_ref, n_est) per program group IN THE ORDER they are summed.  The host
    scorer and `mrmt3.scoring` both assemble their result here."""
    res = {}
    res["Onset precision"], res["Onset recall"], res["Onset F1"] = onset
    sums = {True: [0.0, 0, 0.0, 0], False: [0.0, 0, 0.0, 0]}       # is_drum -> [P*n_est, n_est, R*n_ref, n_ref]
    program_f1 = {}
    for (program, is_drum), (p, r, f), n_ref, n_est in groups:
        if granularity_type == "midi_class":
            program_f1[-1 if is_drum else program] = f
        acc = sums[bool(is_drum)]
        acc[0] += p * n_est
        acc[1] += n_est
        acc[2] += r * n_ref
        acc[3] += n_ref
    p_sum, p_cnt = sums[True][0] + sums[False][0], sums[True][1] + sums[False][1]
    r_sum, r_cnt = sums[True][2] + sums[False][2], sums[True][3] + sums[False][3]
    precision = p_sum / p_cnt if p_cnt else 0
    recall = r_sum / r_cnt if r_cnt else 0
    res.update({f"Onset + program precision ({granularity_type})": precision,
                f"Onset + program recall ({granularity_type})": recall,
                f"Onset + program F1 ({granularity_type})": tm.f_measure(precision, recall),
                "F1 by program": program_f1})
    return res


def group_order(ref_keys, est_keys):
    """The order `mt3_program_aware_note_scores` visits its program groups in: the union of the two key sets, each built
    from its keys in order of first appearance."""
    return list(set(ref_keys) | set(est_keys))


FRAME_KEYS = ("Frame precision", "Frame recall", "Frame F1")
INSTRUMENT_KEYS = ("Num instruments ref", "Num instruments est", "Instrument precision", "Instrument recall", "Instrument F1")


def frame_result(on, grouped):
    """The frame keys from integer counts: `on` the (tp, n_ref, n_est) of the notes "Onset F1" is computed on
    (or None), `grouped` {granularity: [(tp, n_ref, n_est) per program group]}: the counts are summed over the groups, so a
    frame credited to the wrong instrument is one miss and one false alarm.  The host scorer and `mrmt3.scoring` both
    assemble their result here."""
    res = {}
    if on is not None:
        res.update(zip(FRAME_KEYS, tm.scores_from_counts(*on)))
    for name, counts in grouped.items():
        tp, n_ref, n_est = (sum(int(c[i]) for c in counts) for i in range(3))
        res["Frame F1 (%s)" % name] = tm.scores_from_counts(tp, n_ref, n_est)[2]
    return res


def instrument_result(ref_programs, est_programs):
    """The instrument-detection keys from the program numbers of the notes on each side (`tm.instrument_scores`)."""
    return dict(zip(INSTRUMENT_KEYS, tm.instrument_scores(ref_programs, est_programs)))


def _groups(mid, granularity):
    """{(granular program, is_drum): the notes of a file's instruments of that group}, keys in order of first appearance (an
    instrument without notes still names its group)."""
    groups = {}
    for inst in mid.instruments:
        key = (get_granular_program(inst.program, inst.is_drum, granularity), bool(inst.is_drum))
        groups.setdefault(key, []).extend(inst.notes)
    return groups


def _interval_arrays(notes):
    """(intervals f64 [n, 2], MIDI pitches f64 [n]) of a list of notes."""
    return (np.array([[n.start, n.end] for n in notes], dtype=np.float64).reshape(-1, 2),
            np.array([n.pitch for n in notes], dtype=np.float64))


def host_frame_result(ref_mid, est_mid, granularities, on=True):
    """`frame_result` of two MIDI files on the host: "on" from the notes of `tm.sequence_to_valued_intervals`, a
    granularity's groups as `mt3_program_aware_note_scores` forms them, all of their notes."""
    counts = None
    if on:
        iv_r, p_r, _ = tm.sequence_to_valued_intervals(midi_io.midi_to_note_sequence(ref_mid))
        iv_e, p_e, _ = tm.sequence_to_valued_intervals(midi_io.midi_to_note_sequence(est_mid))
        counts = tm.frame_counts(iv_r, p_r, iv_e, p_e)
    grouped = {}
    for g in granularities:
        ref_g, est_g = _groups(ref_mid, g), _groups(est_mid, g)
        grouped[g] = [tm.frame_counts(*_interval_arrays(ref_g.get(key, [])), *_interval_arrays(est_g.get(key, [])))
                      for key in sorted(set(ref_g) | set(est_g)) if ref_g.get(key) or est_g.get(key)]
    return frame_result(counts, grouped)


def _host_instruments(ref_mid, est_mid):
    programs = lambda mid: [inst.program for inst in mid.instruments if inst.notes]
    return instrument_result(programs(ref_mid), programs(est_mid))


def _device_scores(pairs, device, families, with_overlap=True, errors="raise", frames=False, instruments=False):
    from mrmt3 import scoring
    from mrmt3.notes import DeviceNotes
    if instruments and "full" not in families:
        families = tuple(families) + ("full",)
    ref = DeviceNotes.from_arrays([scoring.table_from_midi(_midi(r)) for r, _ in pairs], device)
    est = DeviceNotes.from_arrays([scoring.table_from_midi(_midi(e)) for _, e in pairs], device)
    return scoring.score_tables(ref, est, with_overlap=with_overlap, families=families, errors=errors, frames=frames,
                                instruments=instruments)


def _extra_keys(frames, instruments, granularities=()):
    return ((FRAME_KEYS + tuple("Frame F1 (%s)" % g for g in granularities)) if frames else ()) + (
        INSTRUMENT_KEYS if instruments else ())


def compute_transcription_metrics(ref_mid, est_mid, device=None, frames=False, instruments=False):
    """evaluate.py:25-53: onset+offset and onset-only scores over all notes (pitches are passed to the matcher
    as MIDI numbers, exactly as the reference does).  `device`: the notes are uploaded and matched there
    (`mrmt3.scoring.score_tables`); None is the host matcher.  `frames`: also FRAME_KEYS, the frame score of the same notes
    (DESIGN 4o); `instruments`: also INSTRUMENT_KEYS.  Both paths assemble them from integers in `frame_result` and
    `instrument_result`."""
    ref_mid, est_mid = _midi(ref_mid), _midi(est_mid)
    if device is not None:
        got = _device_scores([(ref_mid, est_mid)], device, ("onoff", "on"), frames=frames, instruments=instruments)[0]
        return {k: got[k] for k in tuple(transcription_metrics_result(0, 0, (0,) * 4, (0,) * 4)) + _extra_keys(frames, instruments)}
    ns_ref = midi_io.midi_to_note_sequence(ref_mid)
    ns_est = midi_io.midi_to_note_sequence(est_mid)
    iv_r, p_r, _ = tm.sequence_to_valued_intervals(ns_ref)
    iv_e, p_e, _ = tm.sequence_to_valued_intervals(ns_est)
    onoff = tm.precision_recall_f1_overlap(iv_r, p_r, iv_e, p_e)
    on = tm.precision_recall_f1_overlap(iv_r, p_r, iv_e, p_e, offset_ratio=None)
    res = transcription_metrics_result(len(iv_r), len(iv_e), onoff, on)
    if frames:
        res.update(host_frame_result(ref_mid, est_mid, ()))
    if instruments:
        res.update(_host_instruments(ref_mid, est_mid))
    return res


def _program_aware_from_scores(got, granularity_type, frames=False, instruments=False):
    keys = ["Onset precision", "Onset recall", "Onset F1"] + [f"Onset + program {k} ({granularity_type})"
                                                              for k in ("precision", "recall", "F1")]
    res = {k: got[k] for k in keys}
    res["F1 by program"] = got["F1 by program (%s)" % granularity_type]
    res.update({k: got[k] for k in _extra_keys(frames, instruments, (granularity_type,))})
    return res


def mt3_program_aware_note_scores(fname1, fname2, granularity_type, device=None, frames=False, instruments=False):
    """evaluate.py:56-237: instrument-agnostic onset F1 plus the program-aware onset F1 of MT3 at the given
    program granularity (per-group scores weighted by note counts).  `device` as in `compute_transcription_metrics`.
    `frames`: also FRAME_KEYS and "Frame F1 (<granularity>)"; `instruments`: also INSTRUMENT_KEYS."""
    ref_mid, est_mid = _midi(fname1), _midi(fname2)
    if device is not None:
        got = _device_scores([(ref_mid, est_mid)], device, ("on", granularity_type), with_overlap=False, frames=frames,
                             instruments=instruments)[0]
        return _program_aware_from_scores(got, granularity_type, frames, instruments)
    iv_r, p_r, _ = tm.sequence_to_valued_intervals(midi_io.midi_to_note_sequence(ref_mid))
    iv_e, p_e, _ = tm.sequence_to_valued_intervals(midi_io.midi_to_note_sequence(est_mid))
    precision, recall, f1, _ = tm.precision_recall_f1_overlap(iv_r, p_r, iv_e, p_e, offset_ratio=None)
    ref_g, est_g = _groups(ref_mid, granularity_type), _groups(est_mid, granularity_type)

    def scored():
        for key in group_order(ref_g, est_g):
            (r_iv, r_pitch), (e_iv, e_pitch) = _interval_arrays(ref_g.get(key, [])), _interval_arrays(est_g.get(key, []))
            p, r, f, _ = tm.precision_recall_f1_overlap(r_iv, tm.midi_to_hz(r_pitch), e_iv, tm.midi_to_hz(e_pitch),
                                                        offset_ratio=None)
            yield key, (p, r, f), len(r_iv), len(e_iv)

    res = program_aware_result((precision, recall, f1), scored(), granularity_type)
    if frames:
        res.update(host_frame_result(ref_mid, est_mid, (granularity_type,)))
    if instruments:
        res.update(_host_instruments(ref_mid, est_mid))
    return res


def loop_transcription_eval(ref_mid, est_mid):
    """evaluate.py:240-272: best onset+offset F1 over estimated tracks for every reference track, averaged."""
    ref_mid, est_mid = _midi(ref_mid), _midi(est_mid)
    score = np.zeros((len(ref_mid.instruments), len(est_mid.instruments)))
    for i, r in enumerate(ref_mid.instruments):
        for j, e in enumerate(est_mid.instruments):
            if r.is_drum != e.is_drum:
                continue
            r_iv = np.array([[n.start, n.end] for n in r.notes]).reshape(-1, 2)
            e_iv = np.array([[n.start, n.end] for n in e.notes]).reshape(-1, 2)
            score[i, j] = tm.precision_recall_f1_overlap(r_iv, tm.midi_to_hz([n.pitch for n in r.notes]), e_iv,
                                                         tm.midi_to_hz([n.pitch for n in e.notes]))[2]
    return float(np.mean(np.max(score, axis=-1))), len(ref_mid.instruments), len(est_mid.instruments)


def evaluate_main(dataset_name, test_midi_dir, ground_truth_midi_dir, enable_instrument_eval=False, first_n=None,
                  device=None, frames=False, instruments=False):
    """evaluate.py:275-330: pair every transcribed file with its ground truth, score at the three program
    granularities, print and return the means.  `device`: the files are read as before, their notes uploaded, and every
    pair is scored in ONE launch of the device matcher (`mrmt3.scoring.score_tables`); None is the host matcher.
    `frames` / `instruments`: the means of the frame keys and of the instrument-detection keys too."""
    if dataset_name == "Slakh":
        est = sorted(glob.glob(f"{test_midi_dir}/*/mix.mid"))
        ref = [k.replace(test_midi_dir, ground_truth_midi_dir).replace("/mix.mid", "/all_src_v2.mid") for k in est]
        if first_n:
            est, ref = est[:first_n], ref[:first_n]
    elif dataset_name in ("ComMU", "NSynth"):
        est = sorted(glob.glob(f"{test_midi_dir}/*.mid"))
        ref = [k.replace(test_midi_dir, ground_truth_midi_dir).replace("_16k.mid", ".mid") for k in est]
    else:
        raise ValueError("dataset_name must be either Slakh or ComMU")

    def score(pair):
        out = {}
        for granularity in ("flat", "full", "midi_class"):
            out.update(mt3_program_aware_note_scores(pair[0], pair[1], granularity, frames=frames, instruments=instruments))
        return out

    scores = collections.defaultdict(list)
    if device is not None:
        mids = []
        for pair in zip(ref, est):
            try:
                mids.append((_midi(pair[0]), _midi(pair[1])))
            except Exception as exc:                      # one unreadable file must not end the run
                print(str(exc))
        families = ("on", "flat", "full", "midi_class")
        for got in (_device_scores(mids, device, families, with_overlap=False, errors="return", frames=frames,
                                   instruments=instruments) if mids else []):
            if isinstance(got, Exception):                # a pair the host matcher would refuse
                print(str(got))
                continue
            out = {}
            for granularity in ("flat", "full", "midi_class"):
                out.update(_program_aware_from_scores(got, granularity, frames, instruments))
            for k, v in out.items():
                scores[k].append(v)
    else:
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
            for fut in concurrent.futures.as_completed([pool.submit(score, p) for p in zip(ref, est)]):
                try:
                    for k, v in fut.result().items():
                        scores[k].append(v)
                except Exception as exc:                      # one unreadable file must not end the run
                    print(str(exc))
    mean_scores = {k: float(np.mean(v)) for k, v in scores.items() if k != "F1 by program"}
    if enable_instrument_eval:
        by_prog = collections.defaultdict(list)
        for d in scores.get("F1 by program", []):
            for prog, f in d.items():
                by_prog[prog].append(f)
        mean_scores["F1 by program"] = {k: float(np.mean(v)) for k, v in sorted(by_prog.items())}
    for k, v in mean_scores.items():
        print(f"{k}: {v}")
    return mean_scores
