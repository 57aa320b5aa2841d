/* mrmt3_hip.h — C ABI of libmrmt3_hip.so: the MI355X (gfx950) kernels of the MR-MT3 hot path.
 *
 * The reference (gudgud96/MR-MT3) is pure Python: this path has NO FFI in the reference.  The
 * boundary it replaces is the chain of stock PyTorch / HuggingFace / torchaudio ops called from
 *   contrib/spectrograms.py:105-145          compute_spectrogram            -> mrmt3_logmel_fwd
 *   models/t5.py:99-180, 478-702             T5Stack wiring over HF T5Block  -> gemm / norm / attn /
 *                                                                              geglu / embed entry points
 *   tasks/mt3_net.py:32-35                   CrossEntropyLoss(ignore=-100)   -> mrmt3_ce_fwd_bwd
 *   tasks/mt3_net.py:54-68                   AdamW + LambdaLR                -> mrmt3_adamw_step
 *   models/t5.py:251-302, t5_segmem_v2_with_prev.py:226-296  greedy generate -> mrmt3_decoder_*
 * Each entry point cites the reference lines it stands for.  INTEGRATION.md shows the ctypes
 * binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - Plain C: pointers are raw DEVICE pointers into caller-owned allocations (torch tensors); sizes
 *    and strides are explicit, in ELEMENTS unless a name ends in _bytes.  No torch types.
 *  - dtype codes: MRMT3_F32 (float) or MRMT3_BF16 (raw bfloat16 bits, uint16_t).  The row, embedding, loss and layout
 *    entry points (norm, geglu, addpos, dropmask_cast, ce, lmhead, cast, transpose) refuse any other code with
 *    MRMT3_ERR_INVALID_ARG before they launch or write anything, also for an operand that is NULL: pass MRMT3_F32 there.
 *  - Every call is asynchronous on the hipStream_t passed as `void* stream`, re-entrant across
 *    streams, never synchronises the device and never allocates (graph-capture safe).  The only
 *    library-owned objects are the opaque mrmt3_decoder handles.
 *  - Dropout: every entry point that draws a mask takes (p_drop, seed, step_dev, stream id): the mask is a pure function
 *    of (seed, stream id, element index) salted, when step_dev is not NULL, by the int32 it points to in DEVICE memory —
 *    read by the kernel at run time, so a captured hipGraph draws new masks every optimizer step (mrmt3_adamw_step
 *    increments the counter; with gradient accumulation the trainer passes a micro-batch counter of its own instead,
 *    bumped by mrmt3_counter_add).  Forward and backward of a site must pass the same four values.
 *  - Return value: 0 = MRMT3_OK, otherwise an error code; mrmt3_last_error() returns a
 *    thread-local message.  Nothing aborts or throws across this ABI.
 */
#ifndef MRMT3_HIP_H
#define MRMT3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRMT3_OK 0
#define MRMT3_ERR_INVALID_ARG 1
#define MRMT3_ERR_HIP 2
#define MRMT3_ERR_UNSUPPORTED 3
#define MRMT3_ERR_COMM 4          /* RCCL missing or a collective call failed */

#define MRMT3_F32 0
#define MRMT3_BF16 1

/* ABI version (major*10000 + minor*100 + patch) and last error text of the calling thread. */
int mrmt3_version(void);
const char* mrmt3_last_error(void);
/* page-locked host memory for tables that reach the device through an async copy (mrmt3_tn_group_run);
 * NULL on failure.  Allocate outside stream capture. */
void* mrmt3_host_alloc(size_t bytes);
void mrmt3_host_free(void* p);

/* Diagnostics: launches per kernel family since the process started (or since the last call with reset != 0).
 * Writes min(n, MRMT3_CNT_N) counters to out and returns MRMT3_CNT_N.  Tests use it to assert that a shape really
 * dispatched to the kernel they mean to check (e.g. the tall-shape ping-pong GEMM needs >= 4096 rows). */
#define MRMT3_CNT_GEMM_NT_TILE 0      /* round-1 256x256 / 256x128 tile kernels (bf16 or exact f32) */
#define MRMT3_CNT_GEMM_NT8 1          /* ping-pong NT kernel */
#define MRMT3_CNT_GEMM_NT_GEGLU 2     /* fused wi + gated-GELU launches (not the two-kernel fallback) */
#define MRMT3_CNT_TN_GROUP 3          /* grouped weight-gradient launches */
#define MRMT3_CNT_TN8 4               /* one-gradient ping-pong TN launches */
#define MRMT3_CNT_TN_TILE 5           /* round-1 128x128 TN kernel */
#define MRMT3_CNT_ATTN_FWD 6          /* bf16 flash forward */
#define MRMT3_CNT_ATTN_BWD 7          /* bf16 flash backward (two-pass: dQ, then dK/dV) */
#define MRMT3_CNT_ATTN_BWD_ONEPASS 8  /* bf16 one-pass backward (keys of a (batch, head) owned by one workgroup) */
#define MRMT3_CNT_ATTN_F32 9          /* exact-f32 attention kernels */
#define MRMT3_CNT_TN_F32 10           /* exact-f32 weight-gradient kernel */
#define MRMT3_CNT_GEMM_NT_SPLITK 11   /* ping-pong NT kernel split over K + reduce (mrmt3_gemm_nt_ws, short inputs) */
#define MRMT3_CNT_GEMM_NT_ADDNORM 12  /* projection + residual add + RMS norm in one launch (mrmt3_gemm_nt_addnorm) */
#define MRMT3_CNT_GEMM_NT_NORMBWD 13  /* data gradient + norm backward in one launch (mrmt3_gemm_nt_normbwd) */
#define MRMT3_CNT_GEMM_NT_GEGLUBWD 14 /* wo data gradient + gated-GELU backward in one launch (mrmt3_gemm_nt_geglubwd) */
#define MRMT3_CNT_ATTN_FWD_VARLEN 15  /* packed-row attention forward, bf16 or exact f32 (mrmt3_attn_fwd_varlen) */
#define MRMT3_CNT_ATTN_BWD_VARLEN 16  /* packed-row attention backward, bf16 or exact f32 (mrmt3_attn_bwd_varlen) */
#define MRMT3_CNT_LOGMEL_WAVE 17      /* log-mel, wave-per-frame kernel (the model's configuration) */
#define MRMT3_CNT_LOGMEL_GENERAL 18   /* log-mel, workgroup-per-frame kernel (every other configuration, MRMT3_LOGMEL=0) */
#define MRMT3_CNT_N 19
int mrmt3_dispatch_counts(unsigned long long* out, int n, int reset);

/* Dispatch / tuning switches ("knobs").  Which kernel or tile shape a call takes is a function of its arguments; a few
 * MRMT3_* environment variables override that choice for A/B measurements and for the parity tests that hold two
 * implementations against each other (MRMT3_ROWS_BM, MRMT3_GEMM8, MRMT3_TN8, MRMT3_LOGMEL, MRMT3_ATTN_ONEPASS, ...; the
 * sources name each one where it is read).  The library reads a knob from the environment ONCE per process, at the first
 * launch that asks for it; later changes of the environment are not seen and no launch path calls getenv again.
 * mrmt3_set_knob(name, value) overrides a knob in-process from the next launch on (name = the variable's name, value = the
 * integer the variable would hold); mrmt3_reset_knobs() drops every override and re-reads the environment at the next use.
 * Process-wide, for tests and tuning: not to be changed while another thread launches. */
int mrmt3_set_knob(const char* name, int value);
int mrmt3_reset_knobs(void);

/* ---- K1: log-mel frontend ---------------------------------------------------------------------
 * contrib/spectrograms.py:92-103,128-145 (pad_end, MelSpectrogram(n_fft 2048, hop, power 1,
 * center False), safe_log) + dataset/dataset_2_random.py:288-289 (clip/scale when normalize!=0)
 * + inference.py:125-126 (frames >= valid_frames[b] are zeroed; valid_frames may be NULL).
 * audio [batch][n_samples] f32 -> out [batch][ceil(n_samples/hop)][n_mels] f32 (or bf16).
 * window [2048] f32; twiddle [1024][2] f32 = exp(-2*pi*i*k/2048); the filterbank is passed in
 * compressed rows: filter m = sum_{q<fb_cnt[m]} fb_w[m*max_taps+q] * |X[fb_start[m]+q]|, fb_w [n_mels][max_taps];
 * what fb_w holds at taps q >= fb_cnt[m] is never used (no zero padding required), 0 <= fb_start[m] <= 1024.
 * Two kernels compute this: the wave-per-frame kernel (n_mels = 512, max_taps <= 12, even hop, fb_start 16-byte and
 * window 8-byte aligned, out 16-byte aligned — the model's configuration) and the general one for everything else;
 * the choice is by these arguments alone and both honour the contract above. */
int mrmt3_logmel_fwd(const float* audio, int batch, int n_samples, int hop, const float* window,
                     const float* twiddle, const int* fb_start, const int* fb_cnt, const float* fb_w,
                     int n_mels, int max_taps, const int* valid_frames, int normalize, int out_bf16,
                     void* out, void* stream);

/* Same frontend for crops gathered out of ONE long recording (the producer side of
 * dataset/dataset_2_random.py:329-344,281-306: _random_chunk picks mel_length frames of the song,
 * _compute_spectrogram runs on those frames alone, _pad_length zero-pads short rows).  Crop b covers
 * samples [seg_start[b], seg_start[b]+n_samples) of audio[total_samples]; it sees zeros past the end
 * of the recording and past valid_frames[b]*hop (its own frames only, never its neighbour's), and
 * output frames >= valid_frames[b] are zero.  seg_start is int64 on the device. */
int mrmt3_logmel_crops_fwd(const float* audio, long long total_samples, const long long* seg_start,
                           int batch, int n_samples, int hop, const float* window,
                           const float* twiddle, const int* fb_start, const int* fb_cnt,
                           const float* fb_w, int n_mels, int max_taps, const int* valid_frames,
                           int normalize, int out_bf16, void* out, void* stream);

/* Same frontend for rows that are MIXED, inside the load that fills the frame, out of stems resident in one device buffer
 * (stem-mix training batches: a random sub-mix of a track's stems at random gains; neither the mix nor the crops are ever
 * materialised).  pool[pool_samples] f32 holds many stems end to end, possibly of several tracks; src_start, src_end
 * (int64) and src_gain (f32) are DEVICE tables [batch][n_src], 1 <= n_src <= 64.  The contract:
 *  - row b, source k: src_start is the pool offset of the crop's first sample, src_end one past the last sample of THAT
 *    STEM.  The source contributes pool[start + i], 0 <= i < n_samples, only while start + i < end: never its neighbour's
 *    samples.
 *  - a source with src_gain == 0.0f is NOT READ AT ALL and its start and end are ignored: this is how a row uses fewer
 *    than n_src stems.
 *  - the kernel never reads outside [0, pool_samples) WHATEVER the tables hold: end is clamped to pool_samples, a source
 *    with start < 0 or start >= end is silent.  A property of the kernel, not a precondition.
 *  - sample i of the row is computed in f32, in source order, the product rounded before the addition (no fused
 *    multiply-add):  acc = 0.f;  for k = 0 .. n_src-1, contributing sources only:  acc = acc + fl(gain_k * sample_k);
 *    one defined f32 value that a sequential numpy restatement reproduces bit for bit.
 *  - the sample is zero for i >= valid_frames[b]*hop and output frames >= valid_frames[b] are zero, as in the crops entry
 *    (valid_frames may be NULL).
 *  - from the mixed sample on it is the frontend above: window, FFT, filterbank, safe log, clamp / scale, f32 or bf16; the
 *    same two kernels by the same argument rule, so with n_src = 1 and gain 1 the output equals mrmt3_logmel_crops_fwd's
 *    bit for bit.
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (valid_frames excepted), n_src outside [1, 64], a size <= 0. */
int mrmt3_logmel_mix_fwd(const float* pool, long long pool_samples, const long long* src_start,
                         const long long* src_end, const float* src_gain, int n_src, int batch, int n_samples,
                         int hop, const float* window, const float* twiddle, const int* fb_start,
                         const int* fb_cnt, const float* fb_w, int n_mels, int max_taps,
                         const int* valid_frames, int normalize, int out_bf16, void* out, void* stream);

/* Windowed-sinc resampler at arbitrary ratio that mixes as it goes (pitch-shift rows of stem-mix training, stems at their
 * native rate, inference on audio at another rate).  It writes rows of f32 SAMPLES, out [batch][n_samples]; the rows then go
 * through mrmt3_logmel_fwd.  pool[pool_samples] f32 as in mrmt3_logmel_mix_fwd; every table below is a DEVICE table
 * [batch][n_src], 1 <= n_src <= 64: src_pos (int64, 32.32 fixed point: the absolute pool position of output sample 0),
 * src_begin / src_end (int64: first sample of the stem, one past its last), src_step (int64, 32.32: input samples per
 * output sample), src_gain (f32), src_filt (int32: which table, or -1).  filt[n_filt][513][n_taps] f32 holds the polyphase
 * tables: P = 512 phases (an ABI constant), row p the taps at a fraction of p/512, row 512 = row 0 shifted by one sample;
 * n_taps is even.  valid_samples [batch] (int64) may be NULL.  The contract, every output one defined f32 value
 * (fl = one rounding to f32; no fused multiply-add, no packed f32):
 *  - output i of source k of row b:  pos = src_pos + i*src_step in int64 (wrapping), n = pos >> 32, fr = pos & 0xffffffff,
 *    j = fr >> 23, w = float(fr & 0x7fffff) * 2^-23 (23 bits: exact).
 *  - tap t has the coefficient  c = fl(h[j][t] + fl(w * fl(h[j+1][t] - h[j][t])))  and reads  idx = n + t - n_taps/2 + 1.
 *  - acc = +0;  for t = 0 .. n_taps-1 in order, only where max(begin, 0) <= idx < min(end, pool_samples):
 *    acc = fl(acc + fl(c * pool[idx])).  A tap outside those bounds is NOT READ and adds nothing (a select, not a product
 *    with zero): what lies between the stems may be NaN.
 *  - the row:  row = +0;  for k = 0 .. n_src-1, sounding sources only:  row = fl(row + fl(gain_k * acc_k)).
 *  - src_filt == -1: no filter.  The source contributes pool[n + i] under the same bounds, the fraction and the step
 *    ignored:  row = fl(row + fl(gain * pool[n + i]))  where that sample exists.  A row whose sources are all -1 is the
 *    mixed row of mrmt3_logmel_mix_fwd bit for bit.
 *  - a source with src_gain == 0.0f is NOT READ AT ALL.  A src_filt outside [-1, n_filt), a step <= 0 or begin >= end makes
 *    the source silent.  Whatever the tables hold, the kernel reads nothing outside [0, pool_samples).
 *  - outputs i >= valid_samples[b] are 0.
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (valid_samples excepted), n_src outside [1, 64], n_taps odd or
 * outside [2, 160], n_filt < 0, a size <= 0, filt not 8-byte aligned.  Checks that name rows are the host's
 * (mrmt3.resample.check_resample_tables). */
int mrmt3_resample_mix_fwd(const float* pool, long long pool_samples, const long long* src_pos,
                           const long long* src_begin, const long long* src_end, const long long* src_step,
                           const float* src_gain, const int* src_filt, int n_src, int batch, int n_samples,
                           const float* filt, int n_filt, int n_taps, const long long* valid_samples, float* out,
                           void* stream);
/* Launches of mrmt3_resample_mix_fwd since the process started (or since the last call with reset != 0): its dispatch
 * counter, kept apart from mrmt3_dispatch_counts so that MRMT3_CNT_N and the counters of an untouched step stay as they are. */
unsigned long long mrmt3_resample_launches(int reset);

/* Stem-mix labels built on the device: the padded target row of every training row, straight from the track's
 * note table, one launch for the whole batch.  A row's targets are by definition Tokenizer.row_targets of the tokenisation
 * of the merged, speed-changed track (mrmt3/stems.py); they are a function of the kept stems' notes, the row's frame window
 * and the speed factor alone, and this entry computes that function.  mrmt3.labels.label_rows_host restates it on the host.
 *
 * The note table (DEVICE, one per track, every stem's notes in stem order; mrmt3.labels.note_table):
 *   note_times [n_notes][2] f64: start and end in seconds, exactly as loaded, finite and >= 0;
 *   note_meta  [n_notes][4] int32, 16-byte aligned: pitch (0..127), velocity bin, program | is_drum << 8 | stem << 16, and
 *     `next`: the index of the note's successor in its (pitch, program, is_drum) group ordered by (start, index) over ALL
 *     stems, -1 for the group's last note.
 * Per row, DEVICE arrays [batch]: keep (uint64, bit s: stem s sounds), start_frame, n_frames, total_frames (int64; the
 * tokenizer's frame count of the stretched track, (n + hop - n % hop) / hop), scale (f64, 2^32 / step), shift (int32,
 * semitones).  The codec and the frames are passed by value: the first token of the pitch, velocity, program and drum
 * ranges and the tie token, max_shift_steps, steps_per_second (sps), sample_rate and hop (frames per second, fps, is their
 * f64 quotient), event_length, num_special_tokens.
 * Nothing bars a different scale and shift in every row.
 *
 * The row (tokens are codec ids; a shift of k steps is the id k):
 *  - Notes: the kept stems' notes in table order.  With shift != 0 a time becomes t * scale in f64, one rounding, and
 *    pitch + shift applies to notes that are not drum notes; with shift == 0 both are untouched.
 *  - Trim: in every (pitch, program, is_drum) group, ordered by start time (equal starts in table order), a note whose end
 *    is greater than its successor's start ends at that start; then notes with start >= end are dropped.  The successor is
 *    the one AMONG THE KEPT STEMS (the kernel follows `next` to the first kept note).
 *  - Events: every note that is not a drum note gives an off event (velocity bin 0) at its end, every note an on event at
 *    its start; ordered by scaled f64 time, off before on, pitched before drum, program, pitch, table index.  The step of
 *    an event is rint(time * steps_per_second), half to even, in f64.
 *  - Window: s0(f) = the largest step s with s / sps <= f / fps, both quotients in f64.  The row's events are those with
 *    s0(start_frame) <= step, and step < s0(start_frame + n_frames) if start_frame + n_frames < total_frames: a row that
 *    ends on the track's last frame takes everything up to the end.
 *  - Tie section: the (program, pitch) pairs whose last event with step < min(s0(start_frame), S_last) is an on event,
 *    S_last the step of the subset's last event, ordered by (program, pitch), emitted as `program, pitch`, then `tie`.
 *    The min restates a quirk of the reference's encode_and_index_events: its state mark stops advancing in the trailing
 *    loop, so a row behind the last note repeats the state before the last step's first event (one note 0.1-0.5 s gives
 *    `program, pitch, tie` for every row after it).
 *  - Walk: the tie section at time 0, then every event emits `program, velocity, pitch`, a drum note `velocity, drum`.  A
 *    velocity or program token equal to the one in force is skipped (the tie section's program tokens count).  Before the
 *    first token an event emits after time has advanced, the shift is written: the time since the row's first step, in
 *    chunks of max_shift_steps, largest first.  Trailing shifts do not exist.
 *  - A kept subset without any event gives `tie` alone (the host tokenizer raises IndexError there).
 *  - targets [batch][event_length] int64 in pad_targets form: truncated to event_length, + num_special_tokens, EOS (1) only
 *    where there is room, -100 behind it.
 * Capacity: a row holds at most 2048 events in its window and 2048 tie pairs (LDS).  A row that needs more is NOT exact
 * and says so: status [batch] int32 is 0 for a row built as above, else a sum of 1 (events over capacity), 2 (tie pairs
 * over capacity), 4 (scaling made two start times of a group equal, so that `next` no longer gives the group's order),
 * 8 (a shifted pitch, a program or a velocity bin outside 0..127; the note is left out).  The caller rebuilds such a row on
 * the host.  Whatever the table holds, the kernel reads nothing outside it and follows at most n_notes links per note.
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (the table's two excepted when n_notes == 0), n_stems outside
 * [1, 64], n_notes < 0, batch, event_length, max_shift_steps, steps_per_second, sample_rate or hop <= 0, a negative
 * token base, note_meta not 16-byte aligned. */
int mrmt3_label_rows_fwd(const double* note_times, const int* note_meta, int n_notes, int n_stems,
                         const unsigned long long* keep, const long long* start_frame, const long long* n_frames,
                         const long long* total_frames, const double* scale, const int* shift, int batch,
                         int pitch_base, int velocity_base, int tie_token, int program_base, int drum_base,
                         int max_shift_steps, int steps_per_second, int sample_rate, int hop, int event_length,
                         int num_special_tokens, long long* targets, int* status, void* stream);
/* Labels of cross-track rows: the row of a VIRTUAL track of up to 4 parts (LB_MAX_PARTS, an ABI constant),
 * each part a track's note table with its own stem mask, speed factor, transposition and delay.  A row's targets are by
 * definition Tokenizer.row_targets of the tokenisation of mrmt3.stems.virtual_note_sequence(parts);
 * mrmt3.labels.label_rows_parts_host restates this entry on the host.
 *
 * The note arena (DEVICE): note_times [n_notes][2] f64 and note_meta [n_notes][4] int32, 16-byte aligned, the note tables
 * of every cached track one after the other, each as mrmt3_label_rows_fwd takes it — but `next` counts from the table's
 * first note, so a table may lie anywhere in the arena.
 * Per (row, part), DEVICE arrays [batch][n_parts]: note_first, note_count (int32: the part's table is notes
 * [note_first, note_first + note_count) of the arena), keep (uint64 stem mask), delay_frames (int64, >= 0; a negative
 * value counts as 0), scale (f64), shift (int32).  Per row, [batch]: start_frame (the virtual track's frame F), n_frames,
 * total_frames (int64, of the virtual track).  The codec by value, as above.  A part with note_count <= 0 or keep == 0
 * contributes nothing.
 *
 * The row is the row of mrmt3_label_rows_fwd over the notes of all parts, with these additions:
 *  - Time of a note of part p: t if shift_p == 0, else fl(t * scale_p); then, if delay_p != 0, fl(that + fl(delay_p / fps)).
 *    One rounding per operation.  Pitch: pitch + shift_p for notes that are not drum notes.
 *  - Trim: the successor of a note is the first kept note along the links of the note's OWN part.  This is the definition's
 *    trim as long as no (program, is_drum) pair is kept in two parts of the row (status 16 otherwise).
 *  - S_last, the tie section and the event list are the row's, over all parts.  In the event order the part index comes
 *    before the index in the part's table.
 *  - status: 1, 2, 4 and 8 as above, the capacities (2048 events, 2048 tie pairs) per row over all parts, 4 also where a
 *    delay made two start times of a group equal; 16: two parts hold kept notes of one (program, is_drum).  The caller
 *    rebuilds a row with status != 0 on the host.
 *  - A one-part row with delay 0 is the row mrmt3_label_rows_fwd writes for that table, integer for integer.
 * Bounds: whatever the arrays and the tables hold, nothing outside [0, n_notes) of the arena is read (a part's range is cut
 * to the arena), a part never follows a link outside its own range, and a note follows at most note_count links.
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (the arena's two excepted when n_notes == 0), n_parts outside
 * [1, 4], n_notes < 0, batch <= 0, the codec checks of mrmt3_label_rows_fwd, note_meta not 16-byte aligned. */
int mrmt3_label_rows_parts_fwd(const double* note_times, const int* note_meta, int n_notes, int n_parts,
                               const int* note_first, const int* note_count, const unsigned long long* keep,
                               const long long* delay_frames, const double* scale, const int* shift,
                               const long long* start_frame, const long long* n_frames, const long long* total_frames,
                               int batch, int pitch_base, int velocity_base, int tie_token, int program_base,
                               int drum_base, int max_shift_steps, int steps_per_second, int sample_rate, int hop,
                               int event_length, int num_special_tokens, long long* targets, int* status, void* stream);
/* Launches of mrmt3_label_rows_fwd and mrmt3_label_rows_parts_fwd since the process started (or since the last call with
 * reset != 0); kept apart from mrmt3_dispatch_counts like the resampler's. */
unsigned long long mrmt3_label_launches(int reset);

/* ---- K2/K4/K6/K7/K9: bias-free Linear layers (nn.Linear(bias=False) inside HF T5Block,
 * models/t5.py:51,72,487-490) ----------------------------------------------------------------------
 * NT:  C[M,N] (+)= A[M,K] . B[N,K]^T      forward y = x W^T, and dgrad with a pre-transposed W.
 * in_dtype applies to A and B; out_dtype to C; accumulate!=0 adds to the existing C (f32 only).
 * Requirements: K*sizeof(in) % 128 == 0; lda/ldb/ldc are row strides in elements. */
int mrmt3_gemm_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N,
                  int K, int in_dtype, int out_dtype, int accumulate, void* stream);
/* The same product with a caller-owned scratch buffer.  Short inputs with a long K (the encoder's 3072 rows at 12
 * segments per GPU: 24-48 tiles for 256 CUs) are cut into 2-4 K ranges that run as tiles of ONE launch — f32 partial sums
 * in the workspace — and are summed in split order by a second kernel (fixed order, no atomics; C bf16 or f32, += for the
 * accumulate form).  mrmt3_gemm_nt_workspace_bytes returns what that takes for a shape, 0 when the shape does not split:
 * then, and with workspace == NULL or too small, the call IS mrmt3_gemm_nt. */
size_t mrmt3_gemm_nt_workspace_bytes(int M, int N, int K, int in_dtype);
int mrmt3_gemm_nt_ws(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                     int in_dtype, int out_dtype, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* TN (weight gradient):  C[N1,N2] (+)= A[M,N1]^T . B[M,N2], bf16 inputs, f32 output, reduction over
 * the M rows split across workgroups; `workspace` must hold mrmt3_gemm_tn_workspace_bytes(...). */
size_t mrmt3_gemm_tn_workspace_bytes(int M, int N1, int N2);
int mrmt3_gemm_tn(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N1,
                  int N2, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The same product in exact f32 (plain FMAs in row order, one writer per element, no workspace): the weight gradients
 * of the fp32 training / parity path — the reference trains at `precision: 32`
 * (config/config_slakh_segmem.yaml:47); torch autograd's `grad_output.t().mm(input)` of nn.Linear. */
int mrmt3_gemm_tn_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N1, int N2,
                      int accumulate, void* stream);
/* Split count of that reduction for a shape: workspace bytes = splits * N1 * N2 * sizeof(float). */
int mrmt3_gemm_tn_splits(int M, int N1, int N2);

/* Grouped form: the weight gradients of several linear layers (one gradient bucket of the backward, or all of it)
 * in ONE MFMA launch + ONE reduce.  Launched one by one a gradient is only 2-16 tiles of 256 x 256, so it has to
 * cut its token rows into 16-32 ranges to occupy the chip and every range leaves a 256-KiB f32 partial tile; together,
 * the items (gradient, token range, tile) are planned on the host so that they fill whole rounds over the CUs with
 * 2-8 ranges per gradient.  The caller keeps A (dY), B (X) alive until the run.  mrmt3_tn_group_plan with
 * table_host == NULL only sizes (info->table_bytes of host+device table, info->slab_bytes of device scratch); with the
 * buffers it writes the table (pointers baked in: re-plan when an address changes), which the caller copies to the
 * device; mrmt3_tn_group_run first copies table_host (page-locked, nullable: table_dev already holds it) to table_dev
 * on `stream` — a memcpy node when the stream is capturing: the replays re-send the same bytes, so table_host must
 * outlive the graph — and launches from the device copy.  Per-element summation order is fixed by the plan
 * (bitwise reproducible for the same plan).  Shapes: mrmt3_tn_group_ok (M >= 1024, N1 % 128 == 0, N2 % 64 == 0,
 * both >= 256, 16-byte aligned rows); everything else goes through mrmt3_gemm_tn. */
typedef struct {
  const void* A;       /* dY [M][lda] bf16 */
  const void* B;       /* X  [M][ldb] bf16 */
  float* C;            /* dW [N1][ldc] f32 */
  int32_t lda, ldb, ldc, M, N1, N2, accumulate, pad;
} mrmt3_tn_gsite;
typedef struct {
  int32_t n_ctas, n_items, n_rtiles, rounds;
  uint64_t rtile_offset, list_offset, sync_offset, table_bytes, slab_bytes;
} mrmt3_tn_group_info;
int mrmt3_tn_group_ok(int M, int N1, int N2, int lda, int ldb, int ldc);
int mrmt3_tn_group_plan(const mrmt3_tn_gsite* sites, int n_sites, void* slab_dev, void* table_host, size_t table_cap,
                        mrmt3_tn_group_info* info);
int mrmt3_tn_group_run(void* table_dev, const void* table_host, const mrmt3_tn_group_info* info, void* stream);

/* ---- K3: T5LayerNorm (RMS norm) fused with the residual add and dropout that precede it --------
 * HF T5LayerNorm + `hidden + dropout(sublayer_out)` (T5LayerSelfAttention/CrossAttention/FF), and
 * models/t5.py:598-601,676-678.
 *   x1 = x0 + dropmask(y)            (y may be NULL: x1 = x0;  x1 may alias x0)
 *   xn = x1 * rsqrt(mean(x1^2)+eps) * w      -> xn (act_dtype), rstd[rows]
 *   out_drop!=0 additionally applies dropout to xn (final_layer_norm + dropout, t5.py:676-678).
 * Dropout masks are regenerated from (seed, stream_id, element index); p==0 disables them. */
int mrmt3_add_rmsnorm_fwd(const float* x0, const void* y, int y_dtype, const float* w, float eps,
                          float* x1, void* xn, int xn_dtype, float* rstd, int rows, int cols,
                          float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_y, uint32_t stream_out,
                          int out_drop, void* stream);
/* backward of the above:
 *   g    = dxn (f32 or bf16, dxn_dtype) [* out-dropout mask]
 *   dx1  = dres (nullable) + rmsnorm_bwd(g; x1, rstd, w)          -> dx1 (may alias dres when the dtypes agree)
 *          dres / dx1 are f32 or — the residual-gradient stream of the bf16 engine, cols == 512 — bf16
 *   dy   = dropmask_y(dx1) as bf16 (nullable)                      -> dy
 *   dw  += sum_rows g * x1 * rstd      (per-workgroup partials in `workspace`, then a 16-way reduction;
 *                                        workspace >= mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, cols))
 *   dw == NULL with a workspace: only the partial rows are written; mrmt3_norm_dw_reduce sums the partial rows of
 *   several such workspaces (one per norm site, all with the same `cols`) into their dw vectors in ONE launch.
 *   `workspaces` / `dws` are DEVICE arrays of n_sites 64-bit addresses, `partial_rows` a device array of
 *   mrmt3_add_rmsnorm_bwd_partial_rows(rows of that site).  Same fixed summation order as the immediate form. */
size_t mrmt3_add_rmsnorm_bwd_workspace_bytes(int rows, int cols);
int mrmt3_add_rmsnorm_bwd_partial_rows(int rows);
int mrmt3_norm_dw_reduce(const void* workspaces, const void* dws, const int* partial_rows, int n_sites, int cols,
                         void* stream);
int mrmt3_add_rmsnorm_bwd(const void* dxn, int dxn_dtype, const void* dres, int dres_dtype, const float* x1,
                          const float* rstd, const float* w, void* dx1, int dx1_dtype, void* dy_bf16,
                          float* dw, int rows, int cols,
                          float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_y, uint32_t stream_out,
                          int out_drop, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K5: attention core (HF T5Attention without relative bias: softmax(q k^T [+causal]) v, scale
 * 1.0, fp32 softmax; models/t5.py:487-490,636-648) -------------------------------------------------
 * q [B][Lq][*] , k/v [B][Lk][*] with head h at columns [h*64, h*64+64) of the row (row strides
 * ldq/ldk/ldv/ldo in elements; batch strides = L*ld).  head_dim is fixed at 64 (d_kv).
 * o [B][Lq][H*64] (ldo), lse [B][H][Lq] f32.  o_lo (nullable, bf16 kernel only, same layout and stride as o) receives
 * bf16(O - bf16(O)), the low half of the f32 output: hand it to mrmt3_attn_bwd and delta = rowsum(dO*O) is formed from
 * O to ~16 bits, which keeps dS = P*(dP - delta) accurate when the value rows share a large common component.
 * causal!=0 masks key > query.  Attention-probability
 * dropout (p_drop) uses a counter hash of (seed, b, h, q, k >> 2), a byte per key.  dtype = MRMT3_BF16 (MFMA flash
 * kernel) or MRMT3_F32 (exact-f32 kernel: fp32 training, parity, decoding prefill; same masks). */
int mrmt3_attn_fwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o,
                   int ldo, void* o_lo, float* lse, int B, int H, int Lq, int Lk, int causal, int dtype,
                   float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);
/* backward of the bf16 kernel: delta [B][H][Lq] f32 scratch is written by the call.
 * dq/dk/dv share the layout (and strides) of q/k/v. */
int mrmt3_attn_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                   const void* o, int ldo, const void* o_lo, const void* d_o, int lddo, const float* lse, float* delta,
                   void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, int B, int H, int Lq,
                   int Lk, int causal, float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);
/* backward of the exact-f32 kernel (autograd of HF T5Attention at `precision: 32`): everything f32, the same masks as
 * the f32 forward; one workgroup per query row (delta, dQ) and per key row (dK, dV), fixed summation order. */
int mrmt3_attn_bwd_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                       int ldo, const float* d_o, int lddo, const float* lse, float* delta, float* dq, int lddq,
                       float* dk, int lddk, float* dv, int lddv, int B, int H, int Lq, int Lk, int causal,
                       float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);

/* The same attention with HF T5Attention's ADDITIVE BIAS (`scores += position_bias`, models/t5.py:636-648: the
 * relative-position bias of stock T5 — SURVEY §8b `attn(q, k, v, bias_or_null, ...)`; MR-MT3's own position_bias is all
 * zeros, models/t5.py:487-490, so the training step never calls these two).  bias: f32 [H][Lq][Lk] shared by the batch
 * (bias_batch_stride = 0) or [B][H][Lq][Lk] (bias_batch_stride = H*Lq*Lk, e.g. a padding mask of -inf / 0 per
 * sequence); NULL = no bias.  dtype = MRMT3_F32 or MRMT3_BF16 operands (q, k, v, o, d_o, dq, dk, dv), f32 arithmetic:
 * this is the general (parity) kernel, one workgroup per query / key row — correct for any bias, not the MFMA fast path.
 * dbias (nullable, layout of bias) receives dS = P (dP - delta); for a shared bias summed over the batch in batch
 * order.  Dropout as above. */
int mrmt3_attn_fwd_bias(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* bias,
                        long long bias_batch_stride, void* o, int ldo, float* lse, int B, int H, int Lq, int Lk,
                        int causal, int dtype, float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id,
                        void* stream);
int mrmt3_attn_bwd_bias(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                        const void* d_o, int lddo, const float* lse, float* delta, const float* bias,
                        long long bias_batch_stride, void* dq, int lddq, void* dk, int lddk, void* dv, int lddv,
                        float* dbias, int B, int H, int Lq, int Lk, int causal, int dtype, float p_drop, uint64_t seed,
                        const int32_t* step_dev, uint32_t stream_id, void* stream);

/* ---- packed decoder rows (training on padded target rows; csrc/pack.hip) ---------------------------------------------
 * A target row padded with -100 (tasks/mt3_net.py:32-35 ignores those positions) only needs its prefix
 * len_b = 1 + (last t with labels[b][t] != -100), 0 for a row without one: under the causal decoder the positions after it
 * reach no scored position and get no gradient.  The prefixes are laid end to end: row b owns packed rows
 * [row_off[b], row_off[b+1]), T = row_off[B], padded to a capacity Tcap >= T (rows [T, Tcap) are the tail).
 * mrmt3_pack_lengths: len [B] int32 from labels [B][L] int64.
 * mrmt3_pack_plan (three small launches, all on the device): len [B], row_off [B+1] int32, per packed row tok_row / tok_pos
 * [Tcap] int32 (row -1 in the tail), dec_ids [Tcap] int64 (the shifted decoder input: start_id at t = 0, labels[b][t-1]
 * otherwise, -100 -> pad_id; pad_id in the tail), targets [Tcap] int64 (labels of the prefix, -100 in the tail), and the
 * tile list of the varlen attention kernels, tiles [2 + 2 * mrmt3_pack_tile_entries(B, Tcap)] int32.  *err (int32) = 1 when
 * T > Tcap: the offsets are then clamped to Tcap and nothing is written past Tcap. */
int mrmt3_pack_tile_entries(int B, int Tcap);
int mrmt3_pack_lengths(const int64_t* labels, int B, int L, int32_t* len, void* stream);
int mrmt3_pack_plan(const int64_t* labels, int B, int L, int Tcap, int start_id, int pad_id, int32_t* len, int32_t* row_off,
                    int32_t* tok_row, int32_t* tok_pos, int64_t* dec_ids, int64_t* targets, int32_t* tiles, int32_t* err,
                    void* stream);
/* embedding of packed rows: x[i] = table[ids[i]] + pos[tok_pos[i]] (ids already shifted: the dec_ids of the plan), dropout
 * keyed by the packed row.  Its backward is mrmt3_embed_bwd with shift = 0 on the same ids. */
int mrmt3_embed_fwd_packed(const int64_t* ids, const int32_t* tok_pos, const float* table, const float* pos, float* x,
                           int rows, int d, int vocab, float p_drop, uint64_t seed, const int32_t* step_dev,
                           uint32_t stream_id, void* stream);
/* attention over packed rows: q / o / dq [Tcap][*] packed by row_off; k / v / dk / dv packed the same way (Lk = 0:
 * self-attention, causal or not) or dense [B][Lk][*] (Lk > 0: cross-attention).  lse / delta [H][Tcap] f32.  Lmax = the
 * longest possible row (the dense L).  For every row the results are those of mrmt3_attn_fwd / mrmt3_attn_bwd (bf16) or the
 * exact-f32 kernels on that row's prefix, with the same dropout masks (keyed by the in-row coordinates (b, h, t_q, t_k));
 * the tail rows of o, o_lo, lse, dq, delta (and dk, dv for self-attention) are written as zeros.  The grid depends on
 * (B, H, Tcap) alone. */
int mrmt3_attn_fwd_varlen(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                          void* o_lo, float* lse, const int32_t* row_off, const int32_t* tiles, int B, int H, int Tcap,
                          int Lmax, int Lk, int causal, int dtype, float p_drop, uint64_t seed, const int32_t* step_dev,
                          uint32_t stream_id, void* stream);
int mrmt3_attn_bwd_varlen(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                          const void* o_lo, const void* d_o, int lddo, const float* lse, float* delta, void* dq, int lddq,
                          void* dk, int lddk, void* dv, int lddv, const int32_t* row_off, const int32_t* tiles, int B, int H,
                          int Tcap, int Lmax, int Lk, int causal, int dtype, float p_drop, uint64_t seed,
                          const int32_t* step_dev, uint32_t stream_id, void* stream);

/* ---- K7: gated-GELU (HF T5DenseGatedGeluDense: gelu_new(h0) * h1, then dropout) ----------------
 * h [rows][2*dff] = [wi_0 x | wi_1 x] -> g [rows][dff] */
int mrmt3_geglu_fwd(const void* h, void* g, int rows, int dff, int dtype, float p_drop,
                    uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);
/* h, dg, dh all of `dtype` (bf16 or f32) */
int mrmt3_geglu_bwd(const void* h, const void* dg, void* dh, int rows, int dff, int dtype, float p_drop,
                    uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);

/* K2 + K7 in one launch (the feed-forward input projection, models/t5.py T5DenseGatedGeluDense.forward):
 * h [rows][ldh >= 2 dff] = x [rows][K] . wi [2 dff][K]^T (bf16, kept for the backward) and
 * g [rows][ldg >= dff] = dropout(gelu_new(h[:, :dff]) * h[:, dff:]).  Bit-identical to mrmt3_gemm_nt followed by
 * mrmt3_geglu_fwd (which is what runs when the shape is outside the fused kernel's: rows < 4096, dff or K not a
 * multiple of 128).  bf16 only. */
int mrmt3_gemm_nt_geglu(const void* x, int ldx, const void* wi, int ldw, void* h, int ldh, void* g, int ldg,
                        int rows, int dff, int K, float p_drop, uint64_t seed, const int32_t* step_dev,
                        uint32_t stream_id, void* stream);

/* ---- A projection and the row kernel behind it in ONE launch (csrc/gemm_rows.hip) ----------------------------------
 * The product's 64-row x 512-column tiles stay on chip (LDS) and the workgroup that computed them runs the row
 * kernel's arithmetic on them: the product's output never makes its HBM round trip.  bf16 operands, model width 512.
 * mrmt3_gemm_rows_ok(M, N, K, lda, ldw): 1 when the fused kernels take the shape (N = 512, or 1024 for the GEGLU
 * backward; K a multiple of 128; row strides multiples of 8 elements; buffers below 2 GiB) — otherwise call the two
 * kernels.
 *
 * mrmt3_gemm_nt_addnorm = mrmt3_gemm_nt (y = A . W^T, [rows][512] bf16) + mrmt3_add_rmsnorm_fwd(x0, y, ...):
 *   x1 = x0 + dropout(y) (f32, may be x0 itself or NULL), xn = w_norm * x1 * rsqrt(mean(x1^2) + eps) (bf16, dropped by
 *   stream_out when out_drop != 0), rstd [rows] (nullable).  HF T5LayerSelfAttention / T5LayerCrossAttention / T5LayerFF:
 *   `hidden + dropout(sublayer(...))` followed by the next sublayer's T5LayerNorm (models/t5.py:636-648).  Same bits as
 *   the two kernels.
 * mrmt3_gemm_nt_normbwd = mrmt3_gemm_nt (dxn = A . WT^T, [rows][512] bf16) + mrmt3_add_rmsnorm_bwd(dxn, dres, ...) with
 *   out_drop = 0: dx1 (f32 or bf16, may be dres itself), dy_bf16 (masked by stream_y, nullable) and — when `workspace`
 *   is given (mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, 512) bytes suffice) — the norm-weight gradient's partial rows,
 *   mrmt3_gemm_nt_normbwd_partial_rows(rows) of them (one per tile of rows), left for mrmt3_norm_dw_reduce.
 * Tile height: 64 rows (two workgroups per CU) until ceil(rows / 128) reaches the CU count, 128 rows (one workgroup per
 * CU, half the weight bytes staged per row) from there on — a function of `rows` alone, so the partial-row count is too.
 * The knob MRMT3_ROWS_BM = 64 / 128 forces one height (parity tests run every case under both).
 * mrmt3_gemm_nt_geglubwd = mrmt3_gemm_nt (dg = dy . WT^T, [rows][dff] bf16, WT = wo^T [dff][K]) + mrmt3_geglu_bwd(h, dg):
 *   dh [rows][2 dff] bf16.  Same bits as the two kernels. */
int mrmt3_gemm_rows_ok(int M, int N, int K, int lda, int ldw);
int mrmt3_gemm_nt_addnorm(const void* A, int lda, const void* W, int ldw, int rows, int K, const float* x0,
                          const float* w_norm, float eps, float* x1, void* xn_bf16, float* rstd, float p_drop,
                          uint64_t seed, const int32_t* step_dev, uint32_t stream_y, uint32_t stream_out, int out_drop,
                          void* stream);
int mrmt3_gemm_nt_normbwd_partial_rows(int rows);
int mrmt3_gemm_nt_normbwd(const void* A, int lda, const void* WT, int ldw, int rows, int K, const void* dres,
                          int dres_dtype, const float* x1, const float* rstd, const float* w_norm, void* dx1,
                          int dx1_dtype, void* dy_bf16, float p_drop, uint64_t seed, const int32_t* step_dev,
                          uint32_t stream_y, void* workspace, size_t workspace_bytes, void* stream);
int mrmt3_gemm_nt_geglubwd(const void* dy, int ldy, const void* WT, int ldw, const void* h, void* dh, int rows, int dff,
                           int K, float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);

/* ---- K8: embedding gather + sinusoid add (+dropout) and its scatter-add backward ---------------
 * models/t5.py:539-540,596-601 and `_shift_right` (t5.py:148-150).
 * ids [rows] int64.  shift!=0 applies HF _shift_right inside the gather: position t of a
 * sequence of length seq_len uses ids[t-1] (start_id at t==0) and maps -100 -> pad_id.
 * x [rows][d] f32 = table[id] + pos[(row % seq_len) + pos_offset], then dropout.
 * pos may be NULL (plain gather, used for the segment-memory ids). */
int mrmt3_embed_fwd(const int64_t* ids, const float* table, const float* pos, float* x, int rows,
                    int seq_len, int d, int vocab, int shift, int start_id, int pad_id,
                    int pos_offset, float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream);
/* dtable[id] += dropmask(dx[row]).  No atomics: rows are ranked by id (counting sort), summed in sorted order and
 * every table row has one writer, so the result is bitwise reproducible and insensitive to how skewed the ids are.
 * workspace >= mrmt3_embed_bwd_workspace_bytes(rows, vocab, d); vocab <= 16384. */
size_t mrmt3_embed_bwd_workspace_bytes(int rows, int vocab, int d);
int mrmt3_embed_bwd(const int64_t* ids, const float* dx, float* dtable, int rows, int seq_len, int d,
                    int vocab, int shift, int start_id, int pad_id, float p_drop, uint64_t seed, const int32_t* step_dev,
                    uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream);
/* x[rows][d] f32 = src[rows][d] (src_dtype) + pos[(row % seq_len)+pos_offset], then dropout
 * (the encoder side of models/t5.py:596-601, input = proj(mel)); backward is dropmask only. */
int mrmt3_addpos_fwd(const void* src, int src_dtype, const float* pos, float* x, int rows, int seq_len,
                     int d, int pos_offset, float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id,
                     void* stream);
/* out (bf16 or f32) = dropmask(dx)  (gradient w.r.t. the GEMM output feeding addpos / any dropout site) */
int mrmt3_dropmask_cast(const float* dx, void* out, int out_dtype, size_t n, float p_drop, uint64_t seed,
                        const int32_t* step_dev, uint32_t stream_id, void* stream);

/* ---- K9: cross-entropy over lm_head logits (tasks/mt3_net.py:32-35; weighted variant :96-108) ---
 * logits [rows][V] f32, targets [rows] int64 (ignore_index -100).  Per row (w_i, n_i) = (1,1) for a
 * normal target, (3,2) for an instrument token in [inst_lo,inst_hi] when weighted!=0 (the
 * reference's `sum_nonpad + 2*sum_inst` over `n_inst + n_nonpad`), (0,0) for ignored rows.
 * mrmt3_ce_count:   denom_dev[0] += sum_i n_i                      (zero it first)
 * mrmt3_ce_fwd_bwd: loss_dev[0]  += sum_i w_i * nll_i / denom      (zero it first; a DOUBLE: one atomic add per
 *                   workgroup in arrival order perturbs it at 1e-16, so the logged float is the same run after run)
 *                   dlogits (nullable, dl_dtype) = grad_scale * w_i * (softmax_i - onehot_i) / denom
 * Both scalars stay on the device: no host synchronisation. */
int mrmt3_ce_count(const int64_t* targets, int rows, int weighted, int inst_lo, int inst_hi,
                   float* denom_dev, void* stream);
int mrmt3_ce_fwd_bwd(const float* logits, const int64_t* targets, const float* denom_dev,
                     double* loss_dev, void* dlogits, int dl_dtype, int rows, int V, int weighted,
                     int inst_lo, int inst_hi, float grad_scale, void* stream);

/* lm_head + cross-entropy without the [rows][V] f32 logits in memory (models/t5.py:72,176-180 followed by
 * tasks/mt3_net.py:32-35).  dec [rows][ld_dec] bf16 = the final-normed decoder states, W [V][ldw] bf16 = lm_head.weight.
 * Rows are processed in chunks of chunk_rows: logits of a chunk = dec_chunk . W^T go (f32) into `workspace`
 * (>= min(rows, chunk_rows)*V*4 bytes, reused by every chunk), then exactly mrmt3_ce_fwd_bwd on that chunk: loss_dev[0]
 * accumulates, dlogits [rows][V] (dl_dtype; nullable: loss only) receives the gradient.  denom_dev as for
 * mrmt3_ce_fwd_bwd (run mrmt3_ce_count over ALL targets first; zero loss_dev first). */
int mrmt3_lmhead_ce_fwd_bwd(const void* dec, int ld_dec, const void* W, int ldw, const int64_t* targets,
                            const float* denom_dev, double* loss_dev, void* dlogits, int dl_dtype, int rows, int V,
                            int d, int weighted, int inst_lo, int inst_hi, float grad_scale, void* workspace,
                            size_t workspace_bytes, int chunk_rows, void* stream);

/* Label smoothing and the T5X z-loss in the same kernels.  Per scored row, with lse = logsumexp(l):
 *   nll_i = lse - l[t],  u_i = lse - mean_j l[j],  r_i = (1 - label_smoothing) * nll_i + label_smoothing * u_i + z_loss * lse^2
 * loss_dev is TWO doubles (zero both first): loss_dev[0] += sum_i w_i * r_i / denom (the objective), loss_dev[1] +=
 * sum_i w_i * nll_i / denom (the plain NLL, what mrmt3_ce_fwd_bwd returns);
 * dlogits = grad_scale * w_i / denom * (softmax_j * (1 + 2 * z_loss * lse) - (1 - label_smoothing) * onehot_j - label_smoothing / V).
 * 0 <= label_smoothing < 1 and z_loss >= 0, anything else is MRMT3_ERR_INVALID_ARG.  Everything else (targets, weights,
 * denom_dev, the chunk loop and its workspace) as for the two entry points above, which are unchanged. */
int mrmt3_ce_fwd_bwd_reg(const float* logits, const int64_t* targets, const float* denom_dev, float label_smoothing,
                         float z_loss, double* loss_dev, void* dlogits, int dl_dtype, int rows, int V, int weighted,
                         int inst_lo, int inst_hi, float grad_scale, void* stream);
int mrmt3_lmhead_ce_fwd_bwd_reg(const void* dec, int ld_dec, const void* W, int ldw, const int64_t* targets,
                                const float* denom_dev, float label_smoothing, float z_loss, double* loss_dev,
                                void* dlogits, int dl_dtype, int rows, int V, int d, int weighted, int inst_lo,
                                int inst_hi, float grad_scale, void* workspace, size_t workspace_bytes, int chunk_rows,
                                void* stream);

/* Teacher-forced scoring, forward only.  mrmt3_token_logprob: out[r] = log softmax(logits[r])[targets[r]], or
 * 0.0 where targets[r] == ignore_index (a target outside [0, V) gives NaN); logits [rows][V] f32, V <= 2048 (an error
 * beyond: the row lives in one wave's registers).  One wave per row: the
 * NaN-propagating row maximum, exp(l - max) summed in f32 per lane in ascending column (lane + 64 i) then by the xor
 * tree, (l[target] - max) - log(sum) -- the arithmetic and order of the decoder's greedy tail.
 * mrmt3_lmhead_logprob: the chunk loop of mrmt3_lmhead_ce_fwd_bwd with that kernel (ignore_index -100): dec [rows][ld_dec]
 * and W [V][ldw] both of `dtype` (MRMT3_BF16 or MRMT3_F32), logits of a chunk (f32) in `workspace`
 * (>= min(rows, chunk_rows)*V*4 bytes); the full [rows][V] logits never exist.  out [rows] f32. */
int mrmt3_token_logprob(const float* logits, const int64_t* targets, float* out, int rows, int V, int ignore_index,
                        void* stream);
int mrmt3_lmhead_logprob(const void* dec, int ld_dec, const void* W, int ldw, const int64_t* targets, float* out,
                         int rows, int V, int d, int dtype, void* workspace, size_t workspace_bytes, int chunk_rows,
                         void* stream);

/* ---- K11: the optimizer tail.  AdamW over the flat parameter buffer (torch.optim.AdamW defaults; tasks/mt3_net.py:55),
 * optionally under the clip coefficient / skip flag of mrmt3_grad_norm (Lightning's `gradient_clip_val` /
 * `gradient_clip_algorithm`, torch.nn.utils.clip_grad_norm_ semantics; the reference passes its `trainer:` block to
 * pl.Trainer, train.py:43-47) and optionally over a table of trainable element ranges (frozen weights, per-range
 * weight decay and learning-rate factor, EMA weights in the same pass).
 * mrmt3_adamw_step: p,g,m,v: flat f32 [n], n % 4 == 0.  lr is read from lr_dev[0] (device), the step count from
 * step_dev[0] (int32, incremented by the call whatever happens: it counts ATTEMPTED optimizer steps).  grad_scale
 * multiplies g (e.g. 1/world_size).  shadow_bf16 (nullable) receives the updated parameters in bf16.
 *   stat_dev non-null (what mrmt3_grad_norm wrote): the gradient is g * grad_scale * stat_dev[1], then, when
 *     clip_value > 0, clamped to [-clip_value, clip_value] (`gradient_clip_algorithm: value`); stat_dev[2] != 0: nothing is
 *     stored (p, m, v, ema and the shadow keep their bits).  With stat_dev[1] == 1 and clip_value == 0 the result is the
 *     plain step's, bit for bit.  clip_value != 0 needs stat_dev.
 *   ranges_dev == NULL and n_ranges == 0: the flat form, one grid-stride launch over all n elements with `weight_decay`;
 *     ema must be NULL and n_trainable is not read.
 *   ranges_dev non-null (n_ranges >= 1; one given without the other is an error): ONE launch over the trainable elements
 *     only (a workgroup owns 1024 consecutive 16-byte groups of the ranges laid end to end and finds its range by binary
 *     search); elements outside every range are never read or written.  Inside a range the arithmetic is the flat form's
 *     with the range's weight decay and lr = lr_dev[0] * lr_scale, bit for bit; `weight_decay` is NOT read.  n_trainable is
 *     what the planner returned (it sizes the grid; the kernel's bound is the table's own total).  With `ema` non-null
 *     (then 0 < ema_decay < 1; ema null needs ema_decay == 0): ema += (1 - ema_decay) * (p_new - ema) in f32 in the same
 *     pass.
 * mrmt3_grad_norm: two launches.  Stage 1 is a FIXED grid (the same on every device and for every n) of 256-thread
 * workgroups that stride over g with 16-byte loads, accumulate g*g in f64 and leave one f64 partial each in `ws`
 * (8-byte aligned, at least mrmt3_grad_norm_workspace_elems() floats; no atomics).  Stage 2, one workgroup, sums the
 * partials in a fixed order in f64 and writes
 *   stat_dev[0] = norm = (float)(sqrt(sum) * grad_scale)      the norm of the gradient AdamW will see, before clipping
 *   stat_dev[1] = coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1      (f32)
 *   stat_dev[2] = skip = 1.0 iff skip_nonfinite and norm is inf or NaN; then also coef = 0 and skipped_dev[0] += 1.
 * The same g gives the same bits wherever it runs.  n % 4 == 0.  ranges_dev / n_ranges as above: NULL and 0 sum all of g;
 * a table sums the elements of its ranges only (a frozen gradient slot is never read), the same fixed grid and summation
 * order over the ranges laid end to end -- a function of the table alone; one range covering the buffer gives the flat
 * form's bits.
 * mrmt3_opt_ranges_plan (host code, no launch): checks `ranges` (sorted, disjoint, bounds multiples of 4 inside [0, n],
 * finite weight_decay / lr_scale >= 0, at least one range) and writes the table the kernels read into `table_host`
 * (mrmt3_opt_ranges_table_bytes(n_ranges) bytes: per range its first 16-byte group, the prefix sum of the groups before it
 * and its two factors, then a sentinel with the total); the caller copies it to the device (8-byte aligned).
 * *n_trainable (nullable) receives the number of elements inside the ranges. */
typedef struct {
  long long begin, end;      /* elements, multiples of 4 */
  float weight_decay, lr_scale;
} mrmt3_opt_range;
size_t mrmt3_opt_ranges_table_bytes(int n_ranges);
int mrmt3_opt_ranges_plan(const mrmt3_opt_range* ranges, int n_ranges, size_t n, void* table_host, size_t table_bytes,
                          size_t* n_trainable);
int mrmt3_adamw_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, const void* ranges_dev,
                     int n_ranges, size_t n_trainable, const float* lr_dev, int32_t* step_dev, float beta1, float beta2,
                     float eps, float weight_decay, float grad_scale, float ema_decay, const float* stat_dev,
                     float clip_value, void* shadow_bf16, void* stream);
size_t mrmt3_grad_norm_workspace_elems(void);
int mrmt3_grad_norm(const float* g, size_t n, const void* ranges_dev, int n_ranges, float grad_scale, float max_norm,
                    int skip_nonfinite, float* ws, size_t ws_elems, float* stat_dev, int32_t* skipped_dev, void* stream);
/* ctr[0] += delta on the device (int32, one thread, stream-ordered).  The trainer's gradient accumulation keeps its
 * per-micro-batch dropout salt in such a counter: it is passed as the step_dev of the dropout entry points and bumped
 * once per micro-batch, inside the captured step, so replays draw new masks per micro-batch. */
int mrmt3_counter_add(int32_t* ctr, int32_t delta, void* stream);
/* out[c][r] = in[r][c] (2-D transpose, with optional f32->bf16 cast) for the pre-transposed dgrad
 * weights. */
int mrmt3_transpose(const void* in, int in_dtype, void* out, int out_dtype, int rows, int cols,
                    void* stream);
int mrmt3_cast(const void* in, int in_dtype, void* out, int out_dtype, size_t n, void* stream);
/* One launch transposes n_mats bf16 matrices living in two flat buffers.  desc_table: device array of
 * {int64 src_off, int64 dst_off, int32 rows, int32 cols} (element offsets; dst is [cols][rows]);
 * tile_start: device int32 prefix sums of ceil(rows/64)*ceil(cols/64), length n_mats. */
int mrmt3_transpose_batched(const void* src_bf16, void* dst_bf16, const void* desc_table,
                            const int* tile_start, int n_mats, int total_tiles, void* stream);

/* ---- K12: greedy decode with a KV cache, one hipGraph replay per token -------------------------
 * models/t5.py:251-302 (batched, MT3Net) and models/t5_segmem_v2_with_prev.py:273-291 (B=1 per
 * segment).  The decoder handle owns: the captured graph, the self-attention KV cache
 * [layers][2][B][max_len][H*64], scratch activations and the device-side step/finished state.
 * Weights are referenced, not copied: `weights` is an array of mrmt3_decoder_weights (device
 * pointers into the caller's flat parameter buffer, dtype = act dtype of the handle).
 * max_batch <= 256 sequences per handle (d_model 512, heads*64 <= 512, d_ff <= 1024). */
typedef struct mrmt3_decoder mrmt3_decoder;
typedef struct {
  const void* embed;        /* [vocab][d] f32 decoder_embed_tokens */
  const float* pos;         /* [>=max_len][d] f32 sinusoid table */
  const void* lm_head;      /* [vocab][d] */
  const float* final_ln;    /* [d] */
  /* per layer l (arrays of n_layers pointers on the HOST): */
  const float* const* ln_self;   /* [d] */
  const void* const* w_qkv;      /* [3*inner][d]  (q|k|v rows) */
  const void* const* w_o_self;   /* [d][inner] */
  const float* const* ln_cross;  /* [d] */
  const void* const* w_q_cross;  /* [inner][d] */
  const void* const* w_o_cross;  /* [d][inner] */
  const float* const* ln_ff;     /* [d] */
  const void* const* w_wi;       /* [2*dff][d]   (wi_0|wi_1 rows) */
  const void* const* w_wo;       /* [d][dff] */
} mrmt3_decoder_weights;

int mrmt3_decoder_create(mrmt3_decoder** out, int n_layers, int d_model, int n_heads, int d_ff,
                         int vocab, int max_batch, int max_len, int max_enc_len, int w_dtype,
                         float eps);
void mrmt3_decoder_destroy(mrmt3_decoder* dec);
/* Start a batch: cross_kv [layers][B*enc_len][2*inner] (k | v columns, dtype = w_dtype) is
 * caller-owned (computed with mrmt3_gemm_nt from the encoder output [+ segment memory]); resets the
 * step counter and finished flags and writes start_id as token 0.  tokens_out [B][max_len+1] int64 is
 * caller-owned.  A row that has emitted eos_id keeps emitting pad_id (models/t5.py:288). */
int mrmt3_decoder_begin(mrmt3_decoder* dec, const mrmt3_decoder_weights* w, const void* cross_kv,
                        int batch, int enc_len, int64_t* tokens_out, int start_id, int eos_id,
                        int pad_id, void* stream);
/* Optional, after mrmt3_decoder_begin: feed n_prefix caller-owned f32 rows per batch row
 * (prefix [batch][n_prefix][d_model], WITHOUT the positional term) as decoder positions
 * 0..n_prefix-1 before the start token, which moves to position n_prefix.  This is
 * T5SegMem.generate_2's memory-prefixed decoder input (models/t5_segmem.py:198-213): the first
 * n_prefix steps of mrmt3_decoder_run only fill the self-attention cache, token steps follow.
 * Needs n_prefix + token steps <= max_len.  mrmt3_decoder_begin clears the prefix. */
int mrmt3_decoder_set_prefix(mrmt3_decoder* dec, const float* prefix, int n_prefix, void* stream);
/* Optional, after mrmt3_decoder_begin: greedy decode with banned tokens.  banned_mask is a caller-owned
 * device [vocab] uint8 (non-zero = banned) or NULL (no ban, the plain argmax).  Banned logits score -inf
 * before the argmax, NaN included (HF's NoBadWordsLogitsProcessor ahead of greedy search).  Switching
 * between a mask and none re-captures the step graph.  mrmt3_decoder_begin clears the ban.
 * Errors in beam mode (the mask is a parameter of mrmt3_decoder_begin_beam there). */
int mrmt3_decoder_set_ban(mrmt3_decoder* dec, const uint8_t* banned_mask, void* stream);
/* Optional, after mrmt3_decoder_begin (and mrmt3_decoder_set_ban) and before mrmt3_decoder_run: greedy decode that also
 * writes the log-probability of every emitted token, out[b][t + 1] beside tokens_out[b][t + 1] (caller-owned device
 * f32 [batch][ld], ld >= max_len + 1; the call writes 0.0 to column 0).  The distribution is the softmax of the logits
 * after the ban (banned entries -inf); a row that had finished writes 0.0 for its pad tokens; prefix steps write
 * nothing; a row whose logits hold a NaN that is not banned writes NaN.  NULL turns it off.  On / off (and the
 * pointer) is part of the captured step's key: switching re-captures, as the ban does; with it off the step is the
 * plain one.  mrmt3_decoder_begin clears it.  Needs vocab <= 2048; errors in beam mode. */
int mrmt3_decoder_set_logprobs(mrmt3_decoder* dec, float* out, int ld, void* stream);
/* Optional, after mrmt3_decoder_begin (and _set_ban / _set_logprobs / _set_prefix) and before mrmt3_decoder_run: the step
 * draws its token instead of taking the argmax (HF 4.18 sample()).  Per row of f32 logits: banned tokens
 * -> -inf; l / temperature (temperature 1 leaves the bits alone); top_k > 0 removes every logit strictly below the
 * min(top_k, vocab)-th largest value (ties with it stay); top_p < 1 keeps token c iff the softmax mass of the tokens
 * with a strictly larger logit is <= top_p (a group of equal logits stays or goes whole; the most likely token always
 * stays); then the lowest column whose cumulative kept probability, in ascending column order, exceeds u * (kept
 * mass), u = 24 random bits / 2^24, a pure function of (seed, batch row b, token step t).  Probabilities are f64.  A
 * row that holds an unbanned NaN, or whose maximum is not finite, emits the greedy token.  Prefix steps draw nothing,
 * finished rows emit pad_id, EOS bookkeeping and the state block are the greedy step's.  With
 * mrmt3_decoder_set_logprobs the value written is the greedy one for the drawn token: log_softmax of the logits after
 * the ban, BEFORE temperature and filters.  The four parameters live in a device record the call writes on `stream`:
 * only "sampling on" is part of the captured step's key, so switching it on or off re-captures and a new seed or new
 * parameters do not.  temperature == 0 switches back to the greedy tail (the other arguments are ignored);
 * mrmt3_decoder_begin clears it.  MRMT3_ERR_INVALID_ARG for temperature < 0 or not finite, top_k < 0, top_p outside
 * (0, 1], vocab > 2048, or in beam mode. */
int mrmt3_decoder_set_sampling(mrmt3_decoder* dec, float temperature, int top_k, float top_p,
                               unsigned long long seed, void* stream);
/* The same rule on caller-owned logits [rows][V] f32 (V <= 2048, an error beyond), by the same device code: row r draws
 * with the counter (row0 + r, step), so (row0 = b, step = t) reproduces row b of a decode at step t.  banned_mask:
 * device [V] uint8 or NULL.  tokens_out [rows] int64; logp_out [rows] f32 (nullable) as above.  temperature > 0. */
int mrmt3_sample_logits(const float* logits, int rows, int V, const uint8_t* banned_mask, float temperature, int top_k,
                        float top_p, unsigned long long seed, int step, int row0, int64_t* tokens_out,
                        float* logp_out, void* stream);
/* Beam search (HF 4.18 beam_search + BeamSearchScorer, early_stopping = False, one hypothesis per group;
 * max_length counts new tokens).  Row r = g * num_beams + j of the batch is beam j of group g; cross_kv
 * holds groups * num_beams rows (each group's K|V repeated num_beams times).  Caller-owned device buffers:
 *   tokens_out  int64 [groups*num_beams][max_len+1]  row r's token of step t at [r][t+1] (start at [r][0])
 *   backptr     int32 [max_len][groups*num_beams][2] {parent row, token} of every row after step t
 *   beam_scores f32   [groups*num_beams]             running beam scores (sums of log-probabilities)
 *   hyps        int32 [groups][32]                   per group: [0] hypotheses held, [1] worst kept score
 *               (f32 bits), [2] done, [3] length of the chosen hypothesis (after finalize), then up to 9
 *               entries {score (f32 bits), end step e, row}: start token + row's tokens of steps 0..e-1.
 * banned_mask: device [vocab] uint8 or NULL; banned tokens score -inf after the log-softmax (whose
 * normaliser still includes them).  Each step appends a select kernel (one workgroup per group: log-softmax,
 * top 2*num_beams of num_beams*vocab, the scorer walk) and a KV-cache reorder kernel to the step graph; a
 * done group emits pad_id.  mrmt3_decoder_run / _poll / _logits work as in greedy mode (state [1] = every
 * group done, [2] = the step it happened).  MRMT3_ERR_INVALID_ARG for num_beams outside 1..8,
 * groups * num_beams > max_batch, or num_beams * vocab * 4 bytes > 64 KiB.  mrmt3_decoder_set_prefix
 * is refused in beam mode. */
int mrmt3_decoder_begin_beam(mrmt3_decoder* dec, const mrmt3_decoder_weights* w, const void* cross_kv,
                             int groups, int num_beams, int enc_len, int64_t* tokens_out, int start_id,
                             int eos_id, int pad_id, float length_penalty, const uint8_t* banned_mask,
                             int32_t* backptr, float* beam_scores, int32_t* hyps, void* stream);
/* After the beam steps (once per decode): BeamSearchScorer.finalize.  Groups not done add their running
 * beams; the best hypothesis of each group (the last added of equal best scores) is read back through the
 * backpointers into out_ids [groups][ld] int64: start token, tokens, eos_id when the hypothesis is
 * shorter than 1 + max_length, pad_id to ld.  hyps[g][3] receives the hypothesis length (start token
 * included, EOS excluded): the caller's output width is min(max over groups + 1, 1 + max_length).
 * A NaN score compares false both ways: a group's first hypothesis stays chosen when its score is NaN, and a NaN
 * further down the list is never chosen.
 * Needs ld >= 1 + max_length and max_length = the number of steps run when a group is not done. */
int mrmt3_decoder_beam_finalize(mrmt3_decoder* dec, int64_t* out_ids, int ld, int max_length, void* stream);
/* The same, and out_logp [groups][ld] f32 (nullable) receives the log-probability of every token of the chosen
 * hypothesis at the token's position: log_softmax of the step's logits (normaliser over the whole vocabulary, as the
 * search scores them), 0.0 for the start token and the padding; the closing eos_id carries its own value when the
 * hypothesis ended with it.  Their sum is the hypothesis' raw score (before the length penalty). */
int mrmt3_decoder_beam_finalize_logprobs(mrmt3_decoder* dec, int64_t* out_ids, float* out_logp, int ld,
                                         int max_length, void* stream);
/* Run n_steps decode steps (graph replays; captured on first use).  No host synchronisation. */
int mrmt3_decoder_run(mrmt3_decoder* dec, int n_steps, void* stream);
/* 1 if the current configuration is being replayed from a captured hipGraph (0 = plain launches). */
int mrmt3_decoder_graph_captured(const mrmt3_decoder* dec);
/* How many step graphs the handle has captured since it was created: a call that changes the captured step's key (batch,
 * pointers, ban / log-probabilities / sampling on or off, greedy or beam) adds one, a replay adds none. */
int mrmt3_decoder_capture_count(const mrmt3_decoder* dec);
/* state_out[0] = steps taken so far, [1] = 1 if every row has emitted EOS, [2] = step index at
 * which the last row finished (or -1); [0] counts prefix positions too, [2] counts token steps only.  Copies 3 int32 asynchronously to caller-owned PINNED host
 * memory; the caller synchronises the stream before reading. */
int mrmt3_decoder_poll(mrmt3_decoder* dec, int32_t* state_out_pinned, void* stream);
/* Stream-ordered device-to-device copy of the logits of the last step run: rows [0, rows) of the
 * f32 [B][vocab] lm_head output (prefix steps included), into caller-owned device memory dst.
 * Errors (MRMT3_ERR_INVALID_ARG) if rows is not in 1..B, before mrmt3_decoder_begin, or inside a
 * stream capture.  For tests: call after mrmt3_decoder_run(dec, 1, stream). */
int mrmt3_decoder_logits(mrmt3_decoder* dec, float* dst, int rows, void* stream);

/* ---- grammar-constrained decoding: only token sequences the MT3 event decoder accepts ----------------
 * The event grammar is a small state machine per decode row, held on the device and advanced inside the captured step by
 * one kernel after the tail (dec_grammar_step); it writes each row's [vocab] uint8 mask (1 = banned) for the next step, which
 * the greedy, sampled and beam tails read where they read the static ban (row stride `vocab` instead of 0).
 * All ids are MODEL ids (the 3 special tokens included); ranges are {first id, count}.  "Off" is the first velocity id. */
typedef struct {
  int shift0, n_shift;        /* shift by v steps = shift0 + v, v in [0, n_shift) */
  int pitch0, n_pitch;        /* n_pitch <= 128 */
  int velocity0, n_velocity;  /* velocity0 = note-off, every other velocity id = on */
  int tie;
  int program0, n_program;    /* n_program <= 128 */
  int drum0, n_drum;
  int eos, pad;
  int max_shift_steps;        /* a shift run may not carry time past this many steps from the segment start */
  int tie_section;            /* 1: a row starts in the tie section, 0: in the body */
  int steps_per_second;       /* the codec's time grid; read by mrmt3_notes_decode_fwd alone (the grammar counts steps) */
} mrmt3_grammar;
#define MRMT3_GRAMMAR_SET_BYTES 2048   /* a 128 x 128 bit set over (program, pitch): bit program * 128 + pitch, LSB first */
/* Stand-alone state (the decoder owns one of its own): `state` is caller-owned device memory of
 * mrmt3_grammar_state_bytes(rows) bytes, 16-byte aligned.  mrmt3_grammar_init writes every row's start state (program and
 * velocity unset, time 0, tie section or body) and its first mask into mask_out [rows][V] uint8.  carry: device
 * [rows][2048] bit sets of the notes sounding when the segment began, or NULL; banned_mask: device [V] uint8 OR-ed into every
 * mask, or NULL.  Both pointers are kept in `state` and read again by mrmt3_grammar_advance: they must stay valid.
 * mrmt3_grammar_advance: row r takes the state of row parents[r] (r itself when parents is NULL), pushes tokens[r] and
 * writes its next mask: the device function of the decoder's step kernel.  `rows` and `V` as given to _init.  A token equal
 * to pad leaves the row's state and mask as they are (row r keeps its own state, whatever parents[r] says).
 * mrmt3_grammar_active copies every row's current `active` set to out [rows][2048]. */
size_t mrmt3_grammar_state_bytes(int rows);
int mrmt3_grammar_init(const mrmt3_grammar* g, void* state, const uint8_t* carry, const uint8_t* banned_mask, int rows,
                       int V, uint8_t* mask_out, void* stream);
int mrmt3_grammar_advance(const mrmt3_grammar* g, void* state, const int32_t* parents_or_null, const int64_t* tokens,
                          int rows, int V, uint8_t* mask_out, void* stream);
int mrmt3_grammar_active(const void* state, int rows, uint8_t* out, void* stream);
/* The `active` set a row of token ids leaves behind: ids [rows][ld] int64 with the start token in column 0; the tokens of
 * columns 1 .. n_tokens (fewer when ld is shorter) are pushed from the start state, up to the first eos or pad.  V: the
 * vocabulary the id ranges must lie in.  carry [rows][2048] or NULL; out [rows][2048].  For rows that were cut after the
 * decode (the segment-memory chains keep max_length columns). */
int mrmt3_grammar_replay(const mrmt3_grammar* g, const int64_t* ids, int ld, int rows, int n_tokens, int V,
                         const uint8_t* carry, uint8_t* out, void* stream);
/* Optional, after mrmt3_decoder_begin / _begin_beam and after mrmt3_decoder_set_ban (the static mask in force is OR-ed
 * into the row masks), before mrmt3_decoder_run: decode under the grammar.  Writes the start state and the step-0 masks;
 * the step graph gains dec_grammar_step and is re-captured when the grammar goes on or off, as for a ban; a new descriptor
 * or carry replays it.  carry: device [rows][2048] (rows = batch, or groups * num_beams) or NULL, valid until the decode
 * ends.  Rows that have finished and the prefix steps of mrmt3_decoder_set_prefix leave state and masks untouched.
 * g = NULL turns it off.  mrmt3_decoder_begin clears it.  Needs n_pitch, n_program <= 128 and every range inside vocab. */
int mrmt3_decoder_set_grammar(mrmt3_decoder* dec, const mrmt3_grammar* g, const uint8_t* carry, void* stream);
/* After the decode (beam: after mrmt3_decoder_beam_finalize): out [rows][2048] receives each row's final `active` set, the
 * notes left sounding by the tokens it emitted (greedy / sampled: rows = batch; beam: rows = groups, the set of the
 * hypothesis returned).  The emitted tokens are pushed again from the start state, so the result does not depend on
 * which rows held the hypothesis' prefix along the way. */
int mrmt3_decoder_grammar_active(mrmt3_decoder* dec, uint8_t* out, void* stream);

/* ---- notes from token rows ---------------------------------------------------------------------------
 * Token rows -> notes on the device: the inverse of mrmt3_label_rows_fwd and the last stage of inference, one
 * launch for every segment of every recording.  The definition is the host decoder as it stands: InferenceHandler's
 * _postprocess_batch + _to_event + contrib.metrics_utils.event_predictions_to_ns (or _scored) with NoteEncodingWithTiesSpec
 * (or ...ScoredSpec); its quirks are reproduced, not repaired.  mrmt3.notes.decode_notes_host restates the contract below on
 * the host.  The result equals the host decoder's note for note, f64 times and f32 scores bit for bit.
 *
 * Input (DEVICE): ids [rows][ld] int64 exactly as the decoder returns them, column 0 the start token; logp [rows][ld] f32
 * beside it or NULL.  Rows are segments; the rows of one recording are contiguous and in time order, seg_first [n_rec + 1]
 * int32 gives each recording's first row (non-decreasing from 0 to rows: the caller checks it; the kernel clamps it).
 * Recordings are independent.  Per row: start_time f64 (the first frame's time minus its remainder mod 1 / steps_per_second)
 * and limit f64, the next row's start_time; any limit <= 0 means "none" (a recording's last row; the host's `if max_time`).
 * g: the id ranges in MODEL ids as for the grammar, plus steps_per_second (max_shift_steps and tie_section are not read: a
 * row always begins in the tie section).  velocity_of_bin [g->n_velocity] int32: the velocity of every velocity id
 * (vocabularies.bin_to_velocity).
 *
 * The row:
 *  - Cut: token j is column j + 1.  The row ends before the first j whose id is g->eos or g->shift0 - 1 (the id that decodes
 *    to -1: UNK, which the host cuts at as well).  A row with no such j contributes NO tokens (the reference's argmax quirk).
 *  - Codec: an id outside the six ranges of g counts 1 invalid event and is skipped (PAD and the extra ids among them).
 *  - Time: a shift of v adds v to `steps`; now = start_time + steps / steps_per_second in f64, one correctly rounded quotient
 *    and one correctly rounded sum, no contraction.  If the row has a limit and now > limit: dropped += (tokens in the row) -
 *    (index of this shift), and the row ends.  Every other event sets steps = 0 and leaves `now` as it is.
 *  - State machine, one per recording, carried from row to row: contrib.note_sequences.decode_note_event exactly.  The tie
 *    section begins at every row's start, also for a row without tokens.  time < current_time counts 1 invalid and changes
 *    nothing; each of the six ValueError sites counts 1 invalid; a re-onset closes the running note first; `tie` ends every
 *    sounding note that was not declared, at current_time; a note's end is max(end, start + 0.01); total_time is the maximum
 *    of the ends; after the last row, current_time = max(current_time, onset + 0.01) over the sounding notes, which then
 *    all end at current_time.
 *  - Order: the host keeps the sounding notes in a dict: `tie` and the flush emit in INSERTION order, and a key that was
 *    popped and struck again has moved to the end.  The notes come out in the host's order.
 *  - Scored (logp != NULL): logc of a note is the f32 the host holds before math.exp: the minimum (taken left to right with
 *    <, as Python's min) over the onset's own token, the row's latest program token, if any, and the row's latest kept
 *    shift token, if any; fixed at the onset for notes that an off, a re-onset, `tie` or the flush emits.
 *
 * Output (DEVICE), per recording r: n_notes, invalid, dropped, status [n_rec] int32; total_time [n_rec] f64; the notes in
 * order from entry seg_first[r] * (ld - 1) of times [rows * (ld - 1)][2] f64 (start, end), meta [rows * (ld - 1)][4] int32
 * (pitch, velocity, program | is_drum << 8, 0: the fields of mrmt3.labels.NoteTable; 16-byte aligned) and, when scored,
 * logc [rows * (ld - 1)] f32.  A recording's notes cannot outnumber its tokens, so a region never overflows; the tail of a
 * region behind n_notes is left unwritten.
 * Capacity: at most MRMT3_NOTES_CAPACITY notes of a recording sound at once (LDS).  A recording that needs more reports
 * status 1 and its other outputs mean nothing: the caller decodes that recording on the host.
 * Whatever the ids hold, the kernel reads and writes nothing outside these arrays, and every loop is bounded by ld, rows or
 * the capacity.
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (logp and logc excepted, which go together), rows, ld or n_rec
 * <= 0, ld < 2, a negative range, n_pitch or n_program > 128, n_velocity <= 0, n_velocity or n_drum > 65536,
 * steps_per_second <= 0, meta not 16-byte aligned. */
#define MRMT3_NOTES_CAPACITY 4096
int mrmt3_notes_decode_fwd(const mrmt3_grammar* g, const long long* ids, const float* logp, int rows, int ld,
                           const int* seg_first, int n_rec, const double* start_time, const double* limit,
                           const int* velocity_of_bin, int* n_notes, int* invalid, int* dropped, int* status,
                           double* total_time, double* times, int* meta, float* logc, void* stream);
/* Launches of mrmt3_notes_decode_fwd since the process started (or since the last call with reset != 0); kept apart from
 * mrmt3_dispatch_counts like the resampler's and the label kernel's. */
unsigned long long mrmt3_notes_launches(int reset);

/* ---- note matching -----------------------------------------------------------------------------------
 * The matcher of the note-level scores on the device: for every problem of one launch a maximum-cardinality matching of
 * the bipartite graph of contrib.transcription_metrics.match_notes (mir_eval's), estimated notes on the left.  Precision,
 * recall and F1 depend on the matching's size alone.  mrmt3.scoring.match_notes_host restates the contract below on the host.
 *
 * Tables (DEVICE): times [n][2] f64 (start, end) and meta [n][4] int32, 16-byte aligned (pitch, velocity,
 * program | is_drum << 8, unused): the fields of mrmt3.labels.NoteTable and of mrmt3_notes_decode_fwd's output, so both feed
 * this kernel as they lie.  Only the times and the pitch are read.
 *
 * Problems: problem p matches the reference entries ref_idx[ref_first[p] .. ref_first[p + 1]) against the estimated entries
 * est_idx[est_first[p] .. est_first[p + 1]); each entry is an index into its table, ref_first / est_first are
 * [n_prob + 1] int32, Lr = ref_first[n_prob], Le = est_first[n_prob].  Each list is in non-decreasing onset order, equal
 * onsets in increasing index order.  A note may appear in many problems: filtering (pitch range, zero durations, program
 * groups) is the caller's, done by choosing the lists; no program field is read.  prob_flags[p]: bit 0 = the offset
 * criterion is on; bits 8 and up = the pitch table used, in [0, n_tables).
 *
 * Edges: f64, one rounding per operation, no contraction.  Reference entry r and estimated entry e are adjacent iff
 *  - rint(|on_r - on_e| * 1e6) / 1e6 <= onset_tol (np.around(., 6): multiply, round half to even, divide), and
 *  - pitch_lo[t][pitch_r] <= pitch_e <= pitch_hi[t][pitch_r], tables [n_tables][128] int32 (pitch_r outside 0..127: no edge;
 *    a table number outside [0, n_tables): a problem without edges), and
 *  - with bit 0: rint(|off_r - off_e| * 1e6) / 1e6 <= max(offset_ratio * (off_r - on_r), offset_min_tol).
 * The pitch tolerance is a table the host computes with the matcher's own expression (mrmt3.scoring.pitch_tables).
 *
 * Output (DEVICE): matched [n_prob] int32, the size of a maximum matching of problem p (unique); match [Le] int32, for
 * estimated entry k the POSITION in ref_idx of its partner or -1: a valid matching of that size, which one is the kernel's
 * choice but the same on every run; status [n_prob] int32: 0 ok, 2 a list of p is not in order (the problem's matched is 0
 * and its match entries are -1 then).
 * An entry whose index lies outside its table, or whose onset is NaN, has no edges and is transparent to the order: the
 * entries around it are compared with each other.  NaN offsets make no edges under bit 0.
 *
 * No capacity: a run of any length is matched in caller-owned device memory, `workspace` of
 * mrmt3_note_match_workspace_bytes(Lr, Le) bytes (4 * Le + 2 * Lr int32; 0 for sizes outside [0, 2^30]), 4-byte aligned,
 * no initial contents needed.  Memory and work are O(entries x window), never O(n_ref * n_est).
 * Whatever the arrays hold, the kernel reads and writes nothing outside them: ref_first / est_first are clamped to
 * [0, Lr] / [0, Le] and made non-decreasing per problem, and every loop is bounded by a list or window length.
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (the workspace included: pass any device pointer when its size
 * is 0), n_prob <= 0, n_tables <= 0 or > 2^22, a note count outside [0, 2^31), a tolerance that is negative or NaN, meta
 * not 16-byte aligned, a workspace not 4-byte aligned. */
size_t mrmt3_note_match_workspace_bytes(long long Lr, long long Le);
int mrmt3_note_match_fwd(const double* ref_times, const int* ref_meta, long long n_ref_notes,
                         const double* est_times, const int* est_meta, long long n_est_notes,
                         const int* ref_idx, const int* ref_first, const int* est_idx, const int* est_first,
                         const int* prob_flags, int n_prob,
                         const int* pitch_lo, const int* pitch_hi, int n_tables,
                         double onset_tol, double offset_ratio, double offset_min_tol,
                         int* matched, int* match, int* status, void* workspace, void* stream);
/* Launches of mrmt3_note_match_fwd since the process started (or since the last call with reset != 0). */
unsigned long long mrmt3_note_match_launches(int reset);

/* ---- frame counts and piano rolls ---------------------------------------------------------------------
 * Both sides of every problem of one launch as time x pitch rolls at `fps` frames a second, and the counts of the frame
 * score: tp = |ref & est|, n_ref = |ref|, n_est = |est| over all 128 pitch rows.  A restatement of the piano-roll
 * convention MT3's frame score stands on (DESIGN 4o says what was and was not checked); the text below is the contract,
 * mrmt3.scoring.frame_counts_host restates it on the host.
 *
 * Tables, lists and `first` arrays are mrmt3_note_match_fwd's (only the times and the pitch are read); the lists need not be
 * in any order.  An entry with times (start, end) and pitch q sounds in frames [a, b) of pitch row q:
 *   a = max(0, floor(start * fps)),  b = max(a + 1, ceil(end * fps)),  both then clamped to [0, n_frames];
 * each product is ONE f64 multiplication (no fused multiply-add, no reciprocal).  A side's roll is the union of its entries.
 * An entry is skipped (it contributes nothing and is counted in skipped[p][side]) when its index lies outside its table,
 * either time is NaN, its pitch lies outside 0..127, or start * fps or end * fps is not below 2^31.  An entry whose b was
 * cut by n_frames is counted in clipped[p][side].  side 0 = reference, 1 = estimate.
 *
 * Output (DEVICE): counts [n_prob][3] int64 (tp, n_ref, n_est), skipped and clipped [n_prob][2] int32, all zeroed on
 * `stream` before the launch; roll: null, or [n_prob][2][128][W] 32-bit words, W = ceil(n_frames / 32), frame f of a row
 * is bit f % 32 of word f / 32; every word is written, the bits at and beyond n_frames are 0.
 * The workspace is not used: mrmt3_note_frames_workspace_bytes returns 0 and `workspace` may be null.
 * Whatever the arrays hold, the kernel reads and writes nothing outside them (`first` clamped as in the matcher).
 * MRMT3_ERR_INVALID_ARG before any launch: a null pointer (roll and the workspace excepted), n_prob <= 0, fps not finite
 * or <= 0, n_frames outside [1, 2^31 - 64], a note count outside [0, 2^31), meta not 16-byte aligned. */
size_t mrmt3_note_frames_workspace_bytes(int n_prob, long long n_frames);
int mrmt3_note_frames_fwd(const double* ref_times, const int* ref_meta, long long n_ref_notes,
                          const double* est_times, const int* est_meta, long long n_est_notes,
                          const int* ref_idx, const int* ref_first, const int* est_idx, const int* est_first,
                          int n_prob, double fps, long long n_frames,
                          long long* counts, int* skipped, int* clipped, unsigned* roll, void* workspace, void* stream);
/* Launches of mrmt3_note_frames_fwd since the process started (or since the last call with reset != 0). */
unsigned long long mrmt3_note_frames_launches(int reset);

/* ---- gradient exchange (data parallel, one process per GPU): RCCL communicators as opaque handles ----------------
 * Replaces what the reference gets from Lightning's `ddp_find_unused_parameters_false` strategy (config/config.yaml:45,
 * train.sh:6): torch DDP's bucketed NCCL all-reduce of the gradients.  The flat f32 gradient buffer is exchanged as a few
 * contiguous buckets (mrmt3/ddp.py), each with one in-place all-reduce on a stream of the caller's choosing.
 * RCCL is resolved at first use (dlopen: $MRMT3_RCCL_LIB, an already mapped librccl, the loader's path, /opt/rocm/lib);
 * the library itself does not link against it.
 *   mrmt3_comm_unique_id : rank 0 fills id_out[MRMT3_COMM_ID_BYTES] and hands the bytes to every other rank (any channel).
 *   mrmt3_comm_create    : every rank, same id; blocks until all `world` ranks have called it.  The GPU the communicator
 *                          is bound to is the calling thread's current HIP device.
 *   mrmt3_allreduce      : buf[0..count) (dtype MRMT3_F32 or MRMT3_BF16, device memory) = sum over ranks, or the mean when
 *                          average != 0; in place, asynchronous on `stream`; every rank must call it with the same count,
 *                          dtype and order of calls.
 *   mrmt3_comm_destroy   : releases the handle (NULL is accepted). */
#define MRMT3_COMM_ID_BYTES 128
int mrmt3_comm_unique_id(void* id_out);
int mrmt3_comm_create(const void* id, int rank, int world, void** comm_out);
int mrmt3_comm_destroy(void* comm);
int mrmt3_allreduce(void* comm, void* buf, size_t count, int dtype, int average, void* stream);

/* Counting hand-offs between two streams whose work is replayed as two separate hipGraphs (the data-parallel step with its
 * all-reduces captured: one graph of compute, one of collectives, mrmt3/trainer.py).  flag / seen / err: int32 in device
 * memory, zero before first use.
 *   mrmt3_flag_signal : *flag += 1 once everything enqueued before it on `stream` has completed (release, device scope).
 *   mrmt3_flag_wait   : `stream` proceeds once *flag >= *seen + 1, then *seen += 1 (only waits on this stream touch seen).
 *                       After timeout_ms without the signal it sets *err = 1 and lets the stream go on: a step whose other
 *                       graph never ran ends in an error word for the host to read, not in a GPU that spins for ever.
 * Both capture into a graph as ordinary kernel nodes; unlike an event-wait node, a wait cannot be satisfied by the previous
 * replay's signal. */
int mrmt3_flag_signal(int32_t* flag, void* stream);
int mrmt3_flag_wait(const int32_t* flag, int32_t* seen, int32_t* err, int timeout_ms, void* stream);

/* ---- capture hygiene (host code that records the training step into hipGraphs: mrmt3/trainer.py) -----------------------
 * The reference's training loop (train.py:99-103, Lightning) has no graph capture; these exist because this path replays the
 * step, and a capture that fails must leave the process able to go on with plain launches (the library never aborts).
 *   mrmt3_stream_capture_status  : 0 = `stream` is not capturing, 1 = capturing, 2 = its capture was invalidated; < 0 = error.
 *   mrmt3_stream_abandon_capture : if `stream` is (still) in capture mode, ends that capture and destroys whatever graph came
 *                                  out of it; clears the calling thread's HIP error slot.  Returns the status BEFORE the call.
 *   mrmt3_runtime_error_pop      : returns (and clears) the calling thread's pending HIP runtime error code — 0 = none — and
 *                                  writes its name to text[0..n).  A launch wrapper of this library reports whatever is in
 *                                  that slot as ITS launch failure, so a host that has just survived a failed HIP call of
 *                                  its own (a refused capture, an RCCL error) empties the slot before launching again.
 *   mrmt3_stream_create / _destroy : a non-blocking stream of the caller's own (priority as hipStreamCreateWithPriority),
 *                                  outside every framework's stream pool: torch's `Stream()` comes round robin out of a pool of 32
 *                                  per priority, and ROCm 7.2 never takes an INVALIDATED stream out of capture mode, so a stream
 *                                  poisoned by one failed capture would come back to a later one.  Destroy only when nothing
 *                                  enqueued on it is pending and no graph is being captured on it.
 *   mrmt3_abort_trace_install    : opt-in diagnostics — on SIGABRT / SIGSEGV write the native frames of the faulting thread to
 *                                  `path` (NULL or "": stderr), then hand the signal to the previous handler. */
int mrmt3_stream_capture_status(void* stream);
int mrmt3_stream_abandon_capture(void* stream);
int mrmt3_runtime_error_pop(char* text, int n);
int mrmt3_stream_create(void** stream_out, int priority);
int mrmt3_stream_destroy(void* stream);
int mrmt3_abort_trace_install(const char* path);

#ifdef __cplusplus
}
#endif
#endif /* MRMT3_HIP_H */
