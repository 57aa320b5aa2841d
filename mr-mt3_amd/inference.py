"""`inference.InferenceHandler` — MI355X drop-in for the reference's inference driver up to token ids
(inference.py:20-215).  Same method names and return conventions; what changed is WHERE things run:

  * `_preprocess`: the padded audio goes to the GPU once and every 256-frame segment's log-mel,
    clip/scale and padded-frame zeroing is ONE `mrmt3_logmel_fwd` launch (the reference computes
    each segment's spectrogram on the CPU main process, rebuilding the filterbank per call).
  * `inference`: `model.generate` is the KV-cached hipGraph decoder; `_postprocess_batch` is
    unchanged arithmetic on the returned ids.
  * `_to_event` / MIDI writing (inference.py:217-234, 195-201): the codec, the run-length decoder and
    the note state machine are restated without note_seq/seqio (`contrib/{event_codec,vocabularies,
    run_length_encoding,note_sequences,metrics_utils,midi_io}.py`); `inference(..., outpath=...)`
    writes a Standard MIDI File and returns the note sequence.
  * `valid_programs` / `num_beams`: the reference passes them to HF `generate` (inference.py:186-190), whose custom
    `generate` then drops them.  Under `decode_options` (knob MRMT3_DECODE_OPTIONS=1) they are honoured:
    `model.generate_beam(..., num_beams, length_penalty=0.4, bad_token_ids=program_ban_ids(valid_programs))`.
  * `with_confidence` / `min_confidence` (not in the reference): the decoder's per-token log-probabilities travel beside the
    tokens and every note gets `confidence` = exp(min(log p)) over its onset token, its segment's program token and the shift
    that set its time; notes below `min_confidence` are dropped.  The MIDI output carries no confidence.
  * `do_sample` / `temperature` / `top_k` / `top_p` / `seed` / `best_of` (the reference's call site pins `do_sample=False`):
    honoured under `decode_options`, like `num_beams`.  Batch i of a recording draws with `seed + i`; `best_of = n` keeps, per
    segment, the most likely of n samples (`model.generate_best_of`, plain T5 only).
  * `device_notes` (not in the reference; off by default): the token ids (and log-probabilities) of all batches stay on the
    device and `_to_event` is replaced by ONE launch of `mrmt3_notes_decode_fwd` per call (`mrmt3.notes.decode_notes`, DESIGN
    §4m); the note sequence is the host path's, note for note.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from contrib import metrics_utils, midi_io, note_sequences, spectrograms, vocabularies

MIN_LOG_MEL = -12
MAX_LOG_MEL = 5
NUM_SPECIAL_TOKENS = 3     # PAD 0 / EOS 1 / UNK 2 (contrib/vocabularies.py:150-171)


def audio_to_frames(audio, spectrogram_config=None):
    """inference.py:64-75 — pads by `hop - len % hop` samples (a full hop when already aligned)."""
    cfg = spectrogram_config or spectrograms.SpectrogramConfig()
    frame_size = cfg.hop_width
    audio = np.pad(audio, [0, frame_size - len(audio) % frame_size], mode='constant')
    frames = spectrograms.split_audio(audio, cfg)
    num_frames = len(audio) // frame_size
    times = np.arange(num_frames) / cfg.frames_per_second
    return frames, times


def split_into_segments(frames, frame_times, max_length=256):
    """inference.py:77-95 — ceil(n/256) zero-padded segments and the count of real frames in each."""
    assert len(frames.shape) >= 1 and frames.shape[0] == frame_times.shape[0]
    num_segment = math.ceil(frames.shape[0] / max_length)
    batchs, times, paddings = [], [], []
    for i in range(num_segment):
        batch = np.zeros((max_length, *frames.shape[1:]))
        t = np.zeros((max_length))
        start = i * max_length
        end = max_length if start + max_length < frames.shape[0] else frames.shape[0] - start
        batch[0:end, ...] = frames[start:start + end, ...]
        t[0:end] = frame_times[start:start + end]
        batchs.append(batch), times.append(t), paddings.append(end)
    return np.stack(batchs, axis=0), np.stack(times, axis=0), paddings


def program_ban_ids(valid_programs, codec=None):
    """Token ids of the programs NOT in `valid_programs`, exactly as the reference's `_get_program_ids`
    (inference.py:138-147) builds its `bad_words_ids`: `p in range(hi - lo)` of the codec's program range (so the
    last program, 127, is never banned), then `vocab.encode` (+ the 3 special tokens)."""
    codec = codec or vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    lo, hi = codec.event_type_range('program')
    valid = set(valid_programs)
    return [lo + p + NUM_SPECIAL_TOKENS for p in range(hi - lo) if p not in valid]


def postprocess_batch(result: torch.Tensor, eos_token_id=1, num_special_tokens=NUM_SPECIAL_TOKENS):
    """inference.py:206-215 — positions at/after the first EOS -> -1, drop the 3 specials, drop BOS."""
    after_eos = torch.cumsum((result == eos_token_id).float(), dim=-1)
    result = result - num_special_tokens
    result = torch.where(after_eos.bool(), -1, result)
    return result[:, 1:].cpu().numpy()


def postprocess_logprobs(logp: torch.Tensor):
    """The log-probabilities that go with `postprocess_batch`'s tokens: the same cut (the BOS column dropped)."""
    return logp[:, 1:].float().cpu().numpy()


class InferenceHandler:
    def __init__(self, model=None, weight_path=None, device=torch.device('cuda'), mel_norm=True,
                 contiguous_inference=False, use_tf_spectral_ops=False, decode_options=None, device_notes=False) -> None:
        if model is None:
            from models.t5 import T5ForConditionalGeneration
            from mrmt3.synthetic import T5_SMALL
            model = T5ForConditionalGeneration(T5_SMALL)
            model.load_state_dict(torch.load(weight_path, map_location='cpu'), strict=True)
            model.eval()
        if use_tf_spectral_ops:
            raise NotImplementedError("TF/ddsp spectral ops are out of scope (SURVEY §2.1 row 1)")
        self.model = model
        self.contiguous_inference = contiguous_inference
        self.SAMPLE_RATE = 16000
        self.spectrogram_config = spectrograms.SpectrogramConfig()
        self.codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))   # inference.py:52-53
        self.device = device
        self.model.to(self.device)
        self.mel_norm = mel_norm
        # honour `valid_programs` / `num_beams` in `inference` (the reference accepts and drops them)
        self.decode_options = bool(int(os.environ.get("MRMT3_DECODE_OPTIONS", "0"))) if decode_options is None \
            else bool(decode_options)
        # tokens -> notes on the device (`_to_notes_device`) instead of `_to_event`; `inference(device_notes=)` overrides it
        self.device_notes = bool(device_notes)

    def _get_program_ids(self, valid_programs):
        """inference.py:138-147: `bad_words_ids` of the programs outside `valid_programs`, one single-token list each."""
        return [[p] for p in program_ban_ids(valid_programs, self.codec)]

    def _generate(self, batch, max_length, valid_programs, num_beams, scored=False, sample=None, best_of=1, constrained=False):
        """The reference's `model.generate(..., num_beams, length_penalty=0.4, bad_words_ids=...)` (inference.py:186-190).
        `scored`: (ids, per-token log-probabilities).  `sample`: dict of `temperature`, `top_k`, `top_p`, `seed` (the
        tokens are drawn; not with `num_beams` > 1); `best_of` > 1: the most likely of that many samples per segment.
        `constrained`: decode under the event grammar (`mrmt3.grammar`)."""
        ban = None if valid_programs is None else program_ban_ids(valid_programs, self.codec)
        ckw = dict(constrained=constrained) if constrained is not False else {}
        if sample is not None:
            if num_beams != 1:
                raise ValueError("beam search does not sample: do_sample / best_of need num_beams == 1")
            if best_of > 1:
                if not hasattr(self.model, "generate_best_of") or getattr(self.model, "VARIANT", "t5") not in ("t5", "segmem_v1"):
                    raise ValueError("best_of > 1 is for the plain T5 model (MT3Net); the segment-memory models decode "
                                     "one sample per segment")
                ids, logp = self.model.generate_best_of(inputs=batch, n=best_of, max_length=max_length, bad_token_ids=ban,
                                                        **sample, **ckw)
                return (ids, logp) if scored else ids
            if ckw:
                from mrmt3.decode import generate_sample
                return generate_sample(self.model, batch, max_length=max_length, bad_token_ids=ban, return_logprobs=scored,
                                       **sample, **ckw)
            return self.model.generate_sample(inputs=batch, max_length=max_length, bad_token_ids=ban,
                                              return_logprobs=scored, **sample)
        if scored:
            return self.model.generate_scored(inputs=batch, max_length=max_length, num_beams=num_beams, length_penalty=0.4,
                                              bad_token_ids=ban, **ckw)
        return self.model.generate_beam(inputs=batch, num_beams=num_beams, max_length=max_length, length_penalty=0.4,
                                        bad_token_ids=ban, **ckw)

    def _audio_to_frames(self, audio):
        return audio_to_frames(audio, self.spectrogram_config)

    def _split_token_into_length(self, frames, frame_times, max_length=256):
        return split_into_segments(frames, frame_times, max_length)

    def _compute_spectrograms(self, inputs, paddings=None):
        """[n_seg, 256, 128] frames -> ([n_seg, 256, 512] log-mel, raw samples); one kernel launch."""
        raw = np.reshape(inputs, (inputs.shape[0], -1))
        x = torch.from_numpy(raw).float().to(self.device)
        vf = None if paddings is None else torch.tensor(paddings, dtype=torch.int32, device=self.device)
        mel = spectrograms.logmel_segments(x, self.spectrogram_config, normalize=self.mel_norm, valid_frames=vf)
        return mel, raw

    def _at_model_rate(self, audio, sample_rate):
        """`audio` at `sample_rate` -> audio at the model's rate: uploaded and resampled on the device
        (mrmt3_resample_mix_fwd).  None, or the model's rate: `audio` itself."""
        if sample_rate is None or sample_rate == self.SAMPLE_RATE:
            return audio
        from mrmt3.resample import resample
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))).to(self.device)
        return resample(x, sample_rate, self.SAMPLE_RATE).cpu().numpy()

    def _preprocess(self, audio):
        frames, frame_times = self._audio_to_frames(audio)
        frames, frame_times, paddings = self._split_token_into_length(frames, frame_times)
        inputs, _ = self._compute_spectrograms(frames, paddings)     # padded frames zeroed in-kernel
        return inputs, frame_times

    def _batching(self, tensors, frame_times, batch_size=5):
        batchs, ft = [], []
        for start in range(0, tensors.shape[0], batch_size):
            end = min(start + batch_size, tensors.shape[0])
            batchs.append(tensors[start:end])
            ft.append(frame_times[start:end])
        return batchs, ft

    def _postprocess_batch(self, result):
        return postprocess_batch(result, self.model.config.eos_token_id)

    def _to_event(self, predictions_np, frame_times, logprobs_np=None, min_confidence=None):
        """inference.py:217-234 — per segment: cut at the first decoded EOS (-1), segment start time =
        first frame time rounded down to the codec step, then decode all segments with ties.
        `logprobs_np` (arrays shaped like `predictions_np`): cut where the tokens are cut, and the notes come back with a
        confidence each, those below `min_confidence` dropped."""
        predictions = []
        for i, batch in enumerate(predictions_np):
            for j, tokens in enumerate(batch):
                # NB (kept from the reference): argmax of an all-False mask is 0, so a segment that
                # never emitted EOS contributes NO tokens.
                n = np.argmax(tokens == vocabularies.DECODED_EOS_ID)
                tokens = tokens[:n]
                start_time = frame_times[i][j][0]
                start_time -= start_time % (1 / self.codec.steps_per_second)
                predictions.append({"est_tokens": tokens, "start_time": start_time, "raw_inputs": []})
                if logprobs_np is not None:
                    predictions[-1]["est_logprobs"] = logprobs_np[i][j][:n]
        if logprobs_np is not None:
            result = metrics_utils.event_predictions_to_ns_scored(
                predictions, codec=self.codec, encoding_spec=note_sequences.NoteEncodingWithTiesScoredSpec,
                min_confidence=min_confidence)
            return result["est_ns"]
        result = metrics_utils.event_predictions_to_ns(predictions, codec=self.codec,
                                                       encoding_spec=note_sequences.NoteEncodingWithTiesSpec)
        return result["est_ns"]

    def _to_notes_device(self, ids, frame_times, logps=None, min_confidence=None, recordings=None, tables=False):
        """`_to_event` on the device: `ids` the decoder's id tensors (one per batch or recording, [rows, width] on the device,
        the widths may differ), `frame_times` their frame times, `logps` the log-probability tensors beside them or None,
        `recordings` the row count of every recording (None: one) -> one note sequence per recording, from one launch.
        `tables`: the notes stay on the device, one `mrmt3.notes.DeviceNotes` for all recordings (unscored)."""
        from mrmt3 import notes
        width = max(t.shape[1] for t in ids)
        eos, pad_id = self.model.config.eos_token_id, getattr(self.model.config, "pad_token_id", 0)
        pad = lambda t, v: t if t.shape[1] == width else torch.nn.functional.pad(t, (0, width - t.shape[1]), value=v)
        # (a row is read up to its first EOS, and a row without one contributes nothing: the padding changes neither)
        flat = torch.cat([pad(t, pad_id) for t in ids])
        if tables:
            return notes.decode_notes_device(flat, np.concatenate(frame_times, axis=0), self.codec, recordings=recordings,
                                             eos_token_id=eos, pad_token_id=pad_id)
        flat_lp = None if logps is None else torch.cat([pad(t.float(), 0.0) for t in logps])
        arrays = notes.decode_notes(flat, np.concatenate(frame_times, axis=0), self.codec, logp=flat_lp, recordings=recordings,
                                    eos_token_id=eos, pad_token_id=pad_id)
        return [a.to_note_sequence(min_confidence) for a in arrays]

    def _sample_options(self, do_sample, temperature, top_k, top_p, seed, best_of):
        """The sampling keywords as `_generate` takes them, or None: honoured only under `decode_options`."""
        if not (isinstance(best_of, int) and best_of >= 1):
            raise ValueError(f"best_of must be an int >= 1, got {best_of!r}")
        if not self.decode_options or not (do_sample or best_of > 1):
            return None
        return dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=int(seed))

    @torch.no_grad()
    def inference(self, audio, audio_path=None, outpath=None, valid_programs=None, num_beams=1, batch_size=5,
                  max_length=1024, verbose=False, return_tokens=False, with_confidence=False, min_confidence=None,
                  do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, best_of=1, constrained=False,
                  sample_rate=None, device_notes=None):
        """audio -> note sequence (and a MIDI file when `outpath` is given, like inference.py:149-204).
        `sample_rate`: the rate of `audio` when it is not the model's 16 kHz (a quarter to four times that): the audio is
        resampled on the device first; None is the 16 kHz path, untouched.
        `return_tokens=True` returns (post-processed token arrays per batch, frame times) instead.
        `with_confidence` (implied by `min_confidence`): every note carries `confidence` in (0, 1], notes below
        `min_confidence` are dropped; with `return_tokens` a third item holds the log-probability arrays.
        `do_sample` (under `decode_options`): the tokens are drawn, batch i with `seed + i`; `best_of` > 1 keeps the most
        likely of that many samples per segment (plain T5 only) and implies sampling.
        `constrained` (under `decode_options`; True or an `EventGrammar`): the decoder emits only tokens the event decoder
        accepts.  The plain T5 decodes a batch's segments side by side, each knowing only its own tie section; the
        segment-memory models hand the sounding notes from segment to segment within a batch.
        `device_notes` (None: the handler's): the tokens become notes on the device, one launch for the whole recording;
        the result is the same note sequence.  `return_tokens` ignores it."""
        scored = with_confidence or min_confidence is not None
        on_device = (self.device_notes if device_notes is None else bool(device_notes)) and not return_tokens
        sample = self._sample_options(do_sample, temperature, top_k, top_p, seed, best_of)
        inputs, frame_times = self._preprocess(self._at_model_rate(audio, sample_rate))
        batches, ft = self._batching(inputs, frame_times, batch_size=batch_size)
        if self.contiguous_inference:
            batches = [torch.cat(batches, dim=0)]
            ft = [np.concatenate(ft, axis=0)]
        results, logps, kept, kept_lp = [], [], [], []
        for i, batch in enumerate(batches):
            kw = {} if sample is None else dict(sample=dict(sample, seed=sample["seed"] + i), best_of=best_of)
            if self.decode_options and constrained is not False:
                kw["constrained"] = constrained
            if scored:
                opts = (valid_programs, num_beams) if self.decode_options else (None, 1)
                result, logp = self._generate(batch.to(self.device), max_length, *opts, scored=True, **kw)
                if on_device:
                    kept_lp.append(logp)
                else:
                    logps.append(postprocess_logprobs(logp))
            elif self.decode_options:
                result = self._generate(batch.to(self.device), max_length, valid_programs, num_beams, **kw)
            else:
                result = self.model.generate(inputs=batch.to(self.device), max_length=max_length)
            if on_device:
                kept.append(result)
            else:
                results.append(self._postprocess_batch(result))
        if return_tokens:
            return (results, ft, logps) if scored else (results, ft)
        if on_device:
            ns = self._to_notes_device(kept, ft, kept_lp if scored else None, min_confidence)[0]
        else:
            ns = self._to_event(results, ft, logps if scored else None, min_confidence)
        if outpath is not None:
            os.makedirs(os.path.dirname(os.path.abspath(outpath)), exist_ok=True)
            midi_io.note_sequence_to_midi_file(ns, outpath)
        return ns

    @torch.no_grad()
    def inference_many(self, audios, outpaths=None, max_length=1024, return_tokens=False, valid_programs=None,
                       num_beams=1, with_confidence=False, min_confidence=None, do_sample=False, temperature=1.0, top_k=0,
                       top_p=1.0, seed=0, best_of=1, constrained=False, sample_rate=None, device_notes=None,
                       return_tables=False):
        """Several recordings in one go (`sample_rate` as in `inference`, the same for every recording).
        Segment-memory models decode them in lockstep (one batch row per
        recording, `model.generate_songs`); the plain T5 simply batches all segments.  Returns one note sequence
        (or, with `return_tokens`, one `(token arrays, frame times)` pair) per recording, like `inference`.
        `valid_programs` / `num_beams` are honoured as given (length penalty 0.4, as `inference` under decode_options).
        `with_confidence` / `min_confidence` as in `inference`.  The sampling keywords as in `inference` (under
        `decode_options`): the plain T5 decodes every segment in one batch under `seed`, the segment-memory models draw
        segment i of every recording under `seed + i`; `best_of` > 1 is for the plain T5.  `constrained` as in `inference`,
        honoured as given.  `device_notes` as in `inference`: every recording's notes come from one launch.
        `return_tables`: the notes are decoded on the device and stay there: one `mrmt3.notes.DeviceNotes` for all
        recordings instead of note sequences, what `mrmt3.scoring.score_tables` takes (no confidence, no files)."""
        if return_tables and (return_tokens or with_confidence or min_confidence is not None or outpaths is not None):
            raise ValueError("return_tables gives the device's note tables alone: no tokens, confidence or MIDI files")
        sample = self._sample_options(do_sample, temperature, top_k, top_p, seed, best_of)
        if sample is not None and best_of > 1 and hasattr(self.model, "generate_songs"):
            raise ValueError("best_of > 1 is for the plain T5 model (MT3Net); the segment-memory models decode one sample "
                             "per segment")
        pre = [self._preprocess(self._at_model_rate(a, sample_rate)) for a in audios]
        opts = valid_programs is not None or num_beams != 1
        scored = with_confidence or min_confidence is not None
        ban = None if valid_programs is None else program_ban_ids(valid_programs, self.codec)
        lps = None
        if hasattr(self.model, "generate_songs"):
            kw = dict(num_beams=num_beams, length_penalty=0.4, bad_token_ids=ban) if opts else {}
            if scored:
                kw["return_logprobs"] = True
            if sample is not None:
                kw.update(sample, do_sample=True, bad_token_ids=ban)
            if constrained is not False:
                kw["constrained"] = constrained
            ids = self.model.generate_songs([x.to(self.device) for x, _ in pre], max_length=max_length, **kw)
            if scored:
                ids, lps = ids
        else:
            x_all = torch.cat([x for x, _ in pre]).to(self.device)
            flat_lp = None
            kw = {} if sample is None else dict(sample=sample, best_of=best_of)
            if constrained is not False:
                kw["constrained"] = constrained
            if scored:
                flat, flat_lp = self._generate(x_all, max_length, valid_programs, num_beams, scored=True, **kw)
            elif opts or sample is not None or constrained is not False:
                flat = self._generate(x_all, max_length, valid_programs, num_beams, **kw)
            else:
                flat = self.model.generate(inputs=x_all, max_length=max_length)
            ids, lps, at = [], ([] if scored else None), 0
            for x, _ in pre:
                ids.append(flat[at:at + x.shape[0]])
                if scored:
                    lps.append(flat_lp[at:at + x.shape[0]])
                at += x.shape[0]
        out = []
        if return_tables:
            return self._to_notes_device(list(ids), [ft for _, ft in pre], recordings=[len(ft) for _, ft in pre], tables=True)
        if (self.device_notes if device_notes is None else bool(device_notes)) and not return_tokens:
            out = self._to_notes_device(list(ids), [ft for _, ft in pre], list(lps) if scored else None, min_confidence,
                                        recordings=[len(ft) for _, ft in pre])
            for k, ns in enumerate(out):
                if outpaths is not None and outpaths[k] is not None:
                    os.makedirs(os.path.dirname(os.path.abspath(outpaths[k])), exist_ok=True)
                    midi_io.note_sequence_to_midi_file(ns, outpaths[k])
            return out
        for k, (seg_ids, (_, ft)) in enumerate(zip(ids, pre)):
            results, times = [self._postprocess_batch(seg_ids)], [ft]
            logps = [postprocess_logprobs(lps[k])] if scored else None
            if return_tokens:
                out.append((results, times, logps) if scored else (results, times))
                continue
            ns = self._to_event(results, times, logps, min_confidence)
            if outpaths is not None and outpaths[k] is not None:
                os.makedirs(os.path.dirname(os.path.abspath(outpaths[k])), exist_ok=True)
                midi_io.note_sequence_to_midi_file(ns, outpaths[k])
            out.append(ns)
        return out
