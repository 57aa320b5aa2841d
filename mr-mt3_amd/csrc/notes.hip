// Token rows -> notes on the device (mrmt3_notes_decode_fwd): the cut at the first EOS, the run-length decoder and
// the note state machine of contrib/note_sequences.py for every segment of every recording in one launch; the contract is the
// header's.  What it writes is a note table (its layout and the alignment check: notetab.h).
//
// One workgroup per recording; it takes the recording's rows in order.  Per row the cut is a strided minimum; then the
// tokens go through LDS in chunks of NT_THREADS: every thread classifies one token, a segmented scan gives the step count
// of every shift, and `now` (one f64 quotient, one f64 sum) is computed for all of them side by side.  Thread 0 then walks
// the chunk: it is the state machine, and all of its state lives in LDS — a map (program, pitch) -> slot and the slots, an
// append-only list, so that slot order IS the insertion order of the host's dict: `tie` and the flush emit by walking it,
// and a popped key leaves a dead slot behind.  `tie` compacts the list while it walks; an onset that finds the list full
// compacts it first, and only if every slot is alive is the recording over capacity.
//
// Integer and f64 work only, one rounding per operation (no fused multiply-add), ordinary vector stores.
#include "notetab.h"

#pragma clang fp contract(off)

#define NT_THREADS 256
#define NT_CAP MRMT3_NOTES_CAPACITY
#define NT_KEYS 16384                            // 128 programs x 128 pitches
#define NT_DEAD 0xffffu

#define NT_INVALID 0
#define NT_SHIFT 1
#define NT_PITCH 2
#define NT_VELOCITY 3
#define NT_TIE 4
#define NT_PROGRAM 5
#define NT_DRUM 6

static_assert(NT_CAP < NT_DEAD, "slot indices are 16-bit");

static MrLaunchCounter g_notes_launches;

// one token of a chunk as the walk reads it: one 16-byte LDS load
struct __attribute__((aligned(16))) NtRec {
  double now;                                    // shifts: the time the shift sets; velocity tokens: the velocity
  float lp;
  int kv;                                        // kind | value << 8
};

struct NtOut {
  double* times;
  int4* meta;
  float* logc;                                   // NULL: not scored
  int n, cap;
  double total;
};

// note_sequences._emit
__device__ __forceinline__ void nt_emit(NtOut& o, double start, double end, int pitch, int velocity, int program, int drum,
                                        float lc) {
  const double least = __dadd_rn(start, 0.01);
  if (least > end) end = least;
  if (o.n < o.cap) {
    o.times[2 * (size_t)o.n] = start;
    o.times[2 * (size_t)o.n + 1] = end;
    o.meta[o.n] = make_int4(pitch, velocity, program | (drum << 8), 0);
    if (o.logc) o.logc[o.n] = lc;
  }
  ++o.n;
  if (end > o.total) o.total = end;
}

__device__ __forceinline__ int nt_classify(const mrmt3_grammar& g, long long id, int& value) {
  const long long s = id - g.shift0, p = id - g.pitch0, v = id - g.velocity0, q = id - g.program0, d = id - g.drum0;
  if (s >= 0 && s < g.n_shift) { value = (int)s; return NT_SHIFT; }
  if (p >= 0 && p < g.n_pitch) { value = (int)p; return NT_PITCH; }
  if (v >= 0 && v < g.n_velocity) { value = (int)v; return NT_VELOCITY; }
  if (id == g.tie) { value = 0; return NT_TIE; }
  if (q >= 0 && q < g.n_program) { value = (int)q; return NT_PROGRAM; }
  if (d >= 0 && d < g.n_drum) { value = (int)d; return NT_DRUM; }
  value = 0;
  return NT_INVALID;
}

__global__ __launch_bounds__(NT_THREADS) void notes_decode_kernel(
    mrmt3_grammar g, const long long* __restrict__ ids, const float* __restrict__ logp, int rows, int ld,
    const int* __restrict__ seg_first, int n_rec, const double* __restrict__ start_time, const double* __restrict__ limit,
    const int* __restrict__ velocity_of_bin, int* __restrict__ n_notes, int* __restrict__ invalid_out,
    int* __restrict__ dropped_out, int* __restrict__ status, double* __restrict__ total_time, double* __restrict__ times,
    int4* __restrict__ meta, float* __restrict__ logc) {
  // the sounding notes: slot_of[program * 128 + pitch] = slot + 1, 0 = not sounding
  __shared__ unsigned short slot_of[NT_KEYS];
  __shared__ double s_onset[NT_CAP];
  __shared__ int s_vel[NT_CAP];
  __shared__ float s_lp[NT_CAP];
  __shared__ unsigned short s_key[NT_CAP];       // NT_DEAD: popped
  __shared__ unsigned char s_tied[NT_CAP];
  // one chunk of a row
  __shared__ long long c_sum[NT_THREADS];
  __shared__ int c_flag[NT_THREADS];
  __shared__ NtRec c_rec[NT_THREADS];
  __shared__ long long s_carry;                  // the step count the next chunk starts from
  __shared__ int s_cut, s_slots, s_stop;         // s_stop: 1 the row has ended (drop), 2 the recording is over capacity

  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  if (r >= n_rec) return;
  const int W = ld - 1;                          // tokens of a row
  int row0 = seg_first[r], row1 = seg_first[r + 1];
  row0 = row0 < 0 ? 0 : (row0 > rows ? rows : row0);
  row1 = row1 < row0 ? row0 : (row1 > rows ? rows : row1);
  const bool scored = logp != nullptr && logc != nullptr;
  const double sps = (double)g.steps_per_second;

  for (int q = tid; q < NT_KEYS; q += NT_THREADS) slot_of[q] = 0;
  if (tid == 0) s_slots = 0;
  int n_slots = 0;                               // thread 0's copy of s_slots, written back at every row's end

  // thread 0's registers: the decoding state (NoteDecodingState) and the counts
  NtOut out;
  out.times = times + 2 * (size_t)row0 * W;
  out.meta = meta + (size_t)row0 * W;
  out.logc = scored ? logc + (size_t)row0 * W : nullptr;
  out.n = 0;
  out.total = 0.0;
  {
    const long long room = (long long)(row1 - row0) * W;
    out.cap = room > 0x7fffffffLL ? 0x7fffffff : (int)room;
  }
  double current_time = 0.0;
  int cur_velocity = 100, cur_program = 0, tie_section = 0;
  long long invalid = 0, dropped = 0;
  bool over = false;

  for (int row = row0; row < row1; ++row) {
    const long long* rid = ids + (size_t)row * ld + 1;
    const float* rlp = scored ? logp + (size_t)row * ld + 1 : nullptr;
    __syncthreads();                             // the previous row's walk is over
    if (tid == 0) {
      s_cut = W;
      s_carry = 0;
      s_stop = over ? 2 : 0;
    }
    for (int q = tid; q < s_slots; q += NT_THREADS) s_tied[q] = 0;      // begin_tied_pitches_section
    __syncthreads();
    int first = W;
    for (int j = tid; j < W; j += NT_THREADS) {
      const long long id = rid[j];
      if (id == g.eos || id == (long long)g.shift0 - 1) { first = j; break; }
    }
    if (first < W) atomicMin(&s_cut, first);
    __syncthreads();
    const int n = s_cut < W ? s_cut : 0;         // no EOS: no tokens
    const double t0 = start_time[row], lim = limit[row];
    // thread 0's per-row state
    tie_section = 1;
    double now = t0;
    float program_lp = 0.f, shift_lp = 0.f;
    bool has_program_lp = false, has_shift_lp = false;

    for (int base = 0; base < n; base += NT_THREADS) {
      if (s_stop) break;                         // (uniform: written before the last barrier)
      const int j = base + tid;
      int kind = NT_INVALID, value = 0;
      if (j < n) kind = nt_classify(g, rid[j], value);
      // steps of every token: the shifts summed since the last event that is neither a shift nor invalid
      long long sum = kind == NT_SHIFT ? value : 0;
      int flag = (j < n && kind != NT_SHIFT && kind != NT_INVALID) ? 1 : 0;
      c_sum[tid] = sum;
      c_flag[tid] = flag;
      for (int off = 1; off < NT_THREADS; off <<= 1) {
        __syncthreads();
        long long a = 0;
        int fa = 0;
        if (tid >= off) { a = c_sum[tid - off]; fa = c_flag[tid - off]; }
        __syncthreads();
        if (tid >= off) {
          if (!flag) sum += a;
          flag |= fa;
          c_sum[tid] = sum;
          c_flag[tid] = flag;
        }
      }
      const long long steps = flag ? sum : sum + s_carry;
      {
        NtRec rec;                               // (a shift's value is not read again: only the others' must fit)
        // (the walk itself reads no global memory: the velocity table is looked up here, by every thread at once)
        rec.now = kind == NT_SHIFT      ? __dadd_rn(t0, __ddiv_rn((double)steps, sps))
                  : kind == NT_VELOCITY ? (double)velocity_of_bin[value]
                                        : 0.0;
        rec.lp = (scored && j < n) ? rlp[j] : 0.f;
        rec.kv = kind | (kind == NT_SHIFT ? 0 : value << 8);
        c_rec[tid] = rec;
      }
      __syncthreads();
      if (tid == NT_THREADS - 1) s_carry = steps;

      if (tid == 0) {
        const int m = n - base < NT_THREADS ? n - base : NT_THREADS;
        NtRec next = c_rec[0];
        for (int t = 0; t < m; ++t) {
          const NtRec rec = next;
          next = c_rec[t + 1 < NT_THREADS ? t + 1 : t];       // in flight while this token is decoded
          const int k = rec.kv & 0xff;
          if (k == NT_INVALID) { ++invalid; continue; }
          if (k == NT_SHIFT) {
            now = rec.now;
            if (lim > 0.0 && now > lim) {
              dropped += n - (base + t);
              s_stop = 1;
              break;
            }
            if (scored) { shift_lp = rec.lp; has_shift_lp = true; }
            continue;
          }
          // decode_note_event(state, now, event)
          if (now < current_time) { ++invalid; continue; }
          const int v = rec.kv >> 8;
          float lc = 0.f;
          if (scored) {                          // min([logprob, program, shift]) as Python takes it
            lc = rec.lp;
            if (has_program_lp && program_lp < lc) lc = program_lp;
            if (has_shift_lp && shift_lp < lc) lc = shift_lp;
          }
          current_time = now;
          if (k == NT_PITCH) {
            const int key = cur_program * 128 + v;
            const int at = slot_of[key];
            if (tie_section) {
              if (!at || s_tied[at - 1]) ++invalid;
              else s_tied[at - 1] = 1;
            } else if (cur_velocity == 0) {
              if (!at) ++invalid;
              else {
                nt_emit(out, s_onset[at - 1], now, v, s_vel[at - 1], cur_program, 0, s_lp[at - 1]);
                s_key[at - 1] = NT_DEAD;
                slot_of[key] = 0;
              }
            } else {
              if (at) {                          // re-onset: close the running note first
                nt_emit(out, s_onset[at - 1], now, v, s_vel[at - 1], cur_program, 0, s_lp[at - 1]);
                s_key[at - 1] = NT_DEAD;
                slot_of[key] = 0;
              }
              int ns = n_slots;
              if (ns == NT_CAP) {                // drop the dead slots; the order stays
                int w = 0;
                for (int q = 0; q < NT_CAP; ++q) {
                  const unsigned kq = s_key[q];
                  if (kq == NT_DEAD) continue;
                  if (w != q) {
                    s_onset[w] = s_onset[q]; s_vel[w] = s_vel[q]; s_lp[w] = s_lp[q]; s_tied[w] = s_tied[q];
                    s_key[w] = (unsigned short)kq;
                    slot_of[kq] = (unsigned short)(w + 1);
                  }
                  ++w;
                }
                ns = w;
              }
              if (ns == NT_CAP) {
                over = true;
                s_stop = 2;
                break;
              }
              s_onset[ns] = now; s_vel[ns] = cur_velocity; s_lp[ns] = lc; s_tied[ns] = 0;
              s_key[ns] = (unsigned short)key;
              slot_of[key] = (unsigned short)(ns + 1);
              n_slots = ns + 1;
            }
          } else if (k == NT_DRUM) {
            if (cur_velocity == 0) ++invalid;
            else nt_emit(out, now, __dadd_rn(now, 0.01), v, cur_velocity, 0, 1, lc);
          } else if (k == NT_VELOCITY) {
            cur_velocity = (int)rec.now;
          } else if (k == NT_PROGRAM) {
            cur_program = v;
            if (scored) { program_lp = rec.lp; has_program_lp = true; }
          } else {                               // NT_TIE
            if (!tie_section) ++invalid;
            else {
              const int ns = n_slots;
              int w = 0;
              for (int q = 0; q < ns; ++q) {
                const unsigned kq = s_key[q];
                if (kq == NT_DEAD) continue;
                if (!s_tied[q]) {
                  nt_emit(out, s_onset[q], current_time, (int)(kq & 127u), s_vel[q], (int)(kq >> 7), 0, s_lp[q]);
                  slot_of[kq] = 0;
                  continue;
                }
                if (w != q) {
                  s_onset[w] = s_onset[q]; s_vel[w] = s_vel[q]; s_lp[w] = s_lp[q]; s_tied[w] = 1;
                  s_key[w] = (unsigned short)kq;
                  slot_of[kq] = (unsigned short)(w + 1);
                }
                ++w;
              }
              n_slots = w;
              tie_section = 0;
            }
          }
        }
      }
      __syncthreads();
    }
    if (tid == 0) s_slots = n_slots;             // (read by everyone behind the next row's first barrier)
  }

  if (tid == 0) {
    if (!over) {                                 // flush_note_decoding_state
      const int ns = n_slots;
      for (int q = 0; q < ns; ++q) {
        if (s_key[q] == NT_DEAD) continue;
        const double least = __dadd_rn(s_onset[q], 0.01);
        if (least > current_time) current_time = least;
      }
      for (int q = 0; q < ns; ++q) {
        const unsigned kq = s_key[q];
        if (kq == NT_DEAD) continue;
        nt_emit(out, s_onset[q], current_time, (int)(kq & 127u), s_vel[q], (int)(kq >> 7), 0, s_lp[q]);
      }
    }
    n_notes[r] = over ? 0 : (out.n < out.cap ? out.n : out.cap);
    invalid_out[r] = (int)invalid;
    dropped_out[r] = (int)dropped;
    status[r] = over ? 1 : 0;
    total_time[r] = out.total;
  }
}

extern "C" int mrmt3_notes_decode_fwd(const mrmt3_grammar* g, const long long* ids, const float* logp, int rows, int ld,
                                      const int* seg_first, int n_rec, const double* start_time, const double* limit,
                                      const int* velocity_of_bin, int* n_notes, int* invalid, int* dropped, int* status,
                                      double* total_time, double* times, int* meta, float* logc, void* stream) {
  MR_CHECK_ARG(g && ids && seg_first && start_time && limit && velocity_of_bin && n_notes && invalid && dropped && status &&
                   total_time && times && meta,
               "notes_decode_fwd: null pointer");
  MR_CHECK_ARG((logp == nullptr) == (logc == nullptr), "notes_decode_fwd: logp and logc go together");
  MR_CHECK_ARG(rows > 0 && n_rec > 0 && ld >= 2, "notes_decode_fwd: rows and n_rec must be > 0 and ld >= 2, got %d, %d, %d",
               rows, n_rec, ld);
  MR_CHECK_ARG(g->shift0 >= 0 && g->n_shift >= 0 && g->pitch0 >= 0 && g->n_pitch >= 0 && g->velocity0 >= 0 &&
                   g->n_velocity > 0 && g->tie >= 0 && g->program0 >= 0 && g->n_program >= 0 && g->drum0 >= 0 &&
                   g->n_drum >= 0,
               "notes_decode_fwd: the id ranges must be >= 0 and n_velocity > 0");
  MR_CHECK_ARG(g->n_pitch <= 128 && g->n_program <= 128, "notes_decode_fwd: n_pitch and n_program must be <= 128, got %d, %d",
               g->n_pitch, g->n_program);
  MR_CHECK_ARG(g->n_drum <= 65536 && g->n_velocity <= 65536, "notes_decode_fwd: n_drum and n_velocity must be <= 65536");
  MR_CHECK_ARG(g->steps_per_second > 0, "notes_decode_fwd: steps_per_second must be > 0, got %d", g->steps_per_second);
  NOTETAB_CHECK_META("notes_decode_fwd", "meta", meta);
  hipLaunchKernelGGL(notes_decode_kernel, dim3((unsigned)n_rec), dim3(NT_THREADS), 0, (hipStream_t)stream, *g, ids, logp, rows,
                     ld, seg_first, n_rec, start_time, limit, velocity_of_bin, n_notes, invalid, dropped, status, total_time,
                     times, (int4*)meta, logc);
  MR_CHECK_LAUNCH("notes_decode_fwd");
  g_notes_launches.hit();
  return MRMT3_OK;
}

extern "C" unsigned long long mrmt3_notes_launches(int reset) { return g_notes_launches.read(reset); }
