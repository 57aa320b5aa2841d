// Stem-mix labels on the device (mrmt3_label_rows_fwd): the padded target row of every training row, straight
// from the track's note table (its layout and the alignment check: notetab.h) — filter, trim, sort, walk; the contract is
// the header's.
//
// One workgroup per row.  Two scans over the table: the first finds the step of the subset's last event (the tie section
// needs it, see the header's quirk), the second marks the sounding (program, pitch) pairs in an LDS bitmap — which is the
// tie section's order for free — and collects the window's events as two-word keys in LDS.  A bitonic sort on the keys, the
// bitmap compacted into a list by a workgroup scan, then thread 0 walks list and events and writes the tokens; everyone
// fills the tail.  A note's trimmed end needs its successor among the kept stems: the table links every note to the next
// of its (pitch, program, is_drum) group over all stems, and a row follows the links to the first kept one.
//
// Integer and f64 work only, one rounding per operation (no fused multiply-add), ordinary vector stores.
#include "notetab.h"

#pragma clang fp contract(off)

#define LB_THREADS 256
#define LB_CAP 2048                              // ABI constant: events of one row's window, and tie-section entries
#define LB_TIE_WORDS 512                         // 128 programs x 128 pitches, one bit each
#define LB_MAX_STEMS 64

#define LB_ST_EVENTS 1
#define LB_ST_TIES 2
#define LB_ST_ORDER 4
#define LB_ST_RANGE 8

static MrLaunchCounter g_label_launches;

struct LbCodec {
  int pitch_base, velocity_base, tie_token, program_base, drum_base, max_shift_steps, sps, event_length, special;
  double fps;
};

// s0(f): the largest step s with s / sps <= f / fps, both quotients in f64 (IEEE division)
__device__ __forceinline__ long long lb_first_step(long long f, double fps, int sps) {
  const double t = (double)f / fps;
  long long s = (long long)floor(t * (double)sps);
  // (the product is off by a step at the most; the caps keep absurd arguments from spinning)
  for (int q = 0; q < 4 && (double)(s + 1) / (double)sps <= t; ++q) ++s;
  for (int q = 0; q < 4 && (double)s / (double)sps > t; ++q) --s;
  return s;
}

__device__ __forceinline__ long long lb_step(double t, int sps) { return (long long)rint(__dmul_rn(t, (double)sps)); }

// f64 -> u64 that orders like the number (times are >= 0; the transform is the general one)
__device__ __forceinline__ unsigned long long lb_time_key(double t) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(t);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double lb_key_time(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct LbNote {
  double start, end;                             // scaled, the end trimmed
  int pitch, vbin, program, drum;
  bool live;
};

// Note i of the table as row (mask, scale, shift) sees it.  flags: LB_ST_* raised by this note.
__device__ __forceinline__ LbNote lb_note(const double* __restrict__ times, const int4* __restrict__ meta, int n_notes, int i,
                                          unsigned long long mask, double scale, int shift, int& flags) {
  LbNote n;
  const int4 m = meta[i];
  n.live = false;
  if (!((mask >> ((m.z >> 16) & 63)) & 1ull)) return n;
  n.drum = (m.z >> 8) & 1;
  n.program = m.z & 0xff;
  n.vbin = m.y;
  n.pitch = (shift != 0 && !n.drum) ? m.x + shift : m.x;
  n.start = times[2 * (size_t)i];
  n.end = times[2 * (size_t)i + 1];
  if (shift != 0) {
    n.start = __dmul_rn(n.start, scale);
    n.end = __dmul_rn(n.end, scale);
  }
  if ((unsigned)n.pitch > 127u || (unsigned)n.program > 127u || (unsigned)n.vbin > 127u) {
    flags |= LB_ST_RANGE;
    return n;
  }
  // the successor among the kept stems (at most n_notes hops, whatever the links hold)
  int j = m.w;
  for (int hops = 0; hops < n_notes && (unsigned)j < (unsigned)n_notes; ++hops) {
    const int zj = meta[j].z;
    if ((mask >> ((zj >> 16) & 63)) & 1ull) break;
    j = meta[j].w;
  }
  if ((unsigned)j < (unsigned)n_notes && ((mask >> ((meta[j].z >> 16) & 63)) & 1ull)) {
    double sj = times[2 * (size_t)j];
    if (shift != 0) {
      sj = __dmul_rn(sj, scale);
      // the links order a group by (unscaled start, index); scaled starts may tie where those did not
      if (sj < n.start || (sj == n.start && j < i)) flags |= LB_ST_ORDER;
    }
    if (n.end > sj) n.end = sj;
  }
  n.live = n.start < n.end;
  return n;
}

__global__ __launch_bounds__(LB_THREADS) void label_rows_kernel(
    const double* __restrict__ times, const int4* __restrict__ meta, int n_notes, const unsigned long long* __restrict__ keep,
    const long long* __restrict__ start_frame, const long long* __restrict__ n_frames,
    const long long* __restrict__ total_frames, const double* __restrict__ scale_b, const int* __restrict__ shift_b,
    int batch, LbCodec c, long long* __restrict__ targets, int* __restrict__ status) {
  __shared__ unsigned long long k_time[LB_CAP], k_ord[LB_CAP];
  __shared__ unsigned tie_bits[LB_TIE_WORDS];
  __shared__ unsigned short tie_list[LB_CAP];
  __shared__ int cnt[LB_THREADS];
  __shared__ long long s_last;
  __shared__ int n_ev, n_tie, n_out, s_flags;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= batch) return;
  const unsigned long long mask = keep[b];
  const double scale = scale_b[b];
  const int shift = shift_b[b];
  const long long f0 = start_frame[b], f1 = f0 + n_frames[b];
  const long long lo = lb_first_step(f0, c.fps, c.sps);
  const long long hi = f1 < total_frames[b] ? lb_first_step(f1, c.fps, c.sps) : 0x7fffffffffffffffLL;

  for (int q = tid; q < LB_TIE_WORDS; q += LB_THREADS) tie_bits[q] = 0u;
  if (tid == 0) {
    s_last = -0x7fffffffffffffffLL;
    n_ev = 0;
    s_flags = 0;
  }
  __syncthreads();

  // scan 1: the step of the subset's last event
  int flags = 0;
  long long last = -0x7fffffffffffffffLL;
  for (int i = tid; i < n_notes; i += LB_THREADS) {
    const LbNote n = lb_note(times, meta, n_notes, i, mask, scale, shift, flags);
    if (!n.live) continue;
    const long long s = lb_step(n.drum ? n.start : n.end, c.sps);      // (start < end: the off event is the later one)
    last = s > last ? s : last;
  }
  atomicMax(&s_last, last);
  __syncthreads();
  const bool any = s_last != -0x7fffffffffffffffLL;
  const long long bound = lo < s_last ? lo : s_last;

  // scan 2: the tie section's pairs and the window's events
  for (int i = tid; any && i < n_notes; i += LB_THREADS) {
    const LbNote n = lb_note(times, meta, n_notes, i, mask, scale, shift, flags);
    if (!n.live) continue;
    const long long s_on = lb_step(n.start, c.sps);
    const unsigned long long ord = ((unsigned long long)n.drum << 62) | ((unsigned long long)n.program << 54) |
                                   ((unsigned long long)n.pitch << 46) | ((unsigned long long)(unsigned)i << 14);
    if (s_on >= lo && s_on < hi) {
      const int slot = atomicAdd(&n_ev, 1);
      if (slot < LB_CAP) {
        k_time[slot] = lb_time_key(n.start);
        k_ord[slot] = ord | (1ull << 63) | (unsigned long long)n.vbin;
      }
    }
    if (!n.drum) {
      const long long s_off = lb_step(n.end, c.sps);
      // a key's events alternate on, off, on, ...: its last event before `bound` is this note's on event iff
      if (s_on < bound && s_off >= bound) atomicOr(&tie_bits[(n.program << 2) | (n.pitch >> 5)], 1u << (n.pitch & 31));
      if (s_off >= lo && s_off < hi) {
        const int slot = atomicAdd(&n_ev, 1);
        if (slot < LB_CAP) {
          k_time[slot] = lb_time_key(n.end);
          k_ord[slot] = ord;
        }
      }
    }
  }
  if (flags) atomicOr(&s_flags, flags);
  __syncthreads();
  const int events = n_ev < LB_CAP ? n_ev : LB_CAP;
  if (tid == 0 && n_ev > LB_CAP) s_flags |= LB_ST_EVENTS;

  // bitonic sort of the events on (time, order), padded with the largest key to a power of two
  int m = 1;
  while (m < events) m <<= 1;
  for (int q = events + tid; q < m; q += LB_THREADS) k_time[q] = k_ord[q] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < m; q += LB_THREADS) {
        const int l = q ^ j;
        if (l > q) {
          const unsigned long long tq = k_time[q], tl = k_time[l], oq = k_ord[q], ol = k_ord[l];
          const bool gt = tq > tl || (tq == tl && oq > ol);
          if (gt == ((q & k) == 0)) {
            k_time[q] = tl; k_time[l] = tq;
            k_ord[q] = ol; k_ord[l] = oq;
          }
        }
      }
      __syncthreads();
    }
  }

  // the bitmap -> the ordered list of (program, pitch) pairs: thread t owns words 2t and 2t + 1
  {
    const unsigned w0 = tie_bits[2 * tid], w1 = tie_bits[2 * tid + 1];
    cnt[tid] = __popc(w0) + __popc(w1);
    __syncthreads();
    int at = 0;
    for (int q = 0; q < tid; ++q) at += cnt[q];
    if (tid == LB_THREADS - 1) n_tie = at + cnt[tid];
    for (int h = 0; h < 2; ++h) {
      unsigned w = h ? w1 : w0;
      while (w) {
        const int bit = __ffs(w) - 1;
        w &= w - 1;
        if (at < LB_CAP) tie_list[at] = (unsigned short)(((2 * tid + h) << 5) | bit);   // = program << 7 | pitch
        ++at;
      }
    }
  }
  __syncthreads();

  // the walk
  const int L = c.event_length;
  long long* out = targets + (size_t)b * L;
  if (tid == 0) {
    int n = 0, cur_program = -1, cur_velocity = -1;
    const int ties = n_tie < LB_CAP ? n_tie : LB_CAP;
    if (n_tie > LB_CAP) s_flags |= LB_ST_TIES;
    for (int t = 0; t < ties && n < L; ++t) {
      const int program = tie_list[t] >> 7, pitch = tie_list[t] & 127;
      if (program != cur_program) {
        out[n++] = c.program_base + program + c.special;
        cur_program = program;
      }
      if (n < L) out[n++] = c.pitch_base + pitch + c.special;
    }
    if (n < L) out[n++] = c.tie_token + c.special;
    long long flushed = 0;
    for (int e = 0; e < events && n < L; ++e) {
      const unsigned long long o = k_ord[e];
      const int on = (int)(o >> 63), drum = (int)(o >> 62) & 1, program = (int)(o >> 54) & 0xff,
                pitch = (int)(o >> 46) & 0xff, vbin = on ? (int)(o & 0x3fff) : 0;
      const long long total = lb_step(lb_key_time(k_time[e]), c.sps) - lo;
      if (total > flushed) {                     // every event emits its pitch or drum token: the shift comes first
        flushed = total;
        for (long long left = total; left > 0 && n < L;) {
          const long long chunk = left < c.max_shift_steps ? left : c.max_shift_steps;
          out[n++] = chunk + c.special;
          left -= chunk;
        }
      }
      if (!drum && program != cur_program) {
        if (n < L) out[n++] = c.program_base + program + c.special;
        cur_program = program;
      }
      if (vbin != cur_velocity) {
        if (n < L) out[n++] = c.velocity_base + vbin + c.special;
        cur_velocity = vbin;
      }
      if (n < L) out[n++] = (drum ? c.drum_base : c.pitch_base) + pitch + c.special;
    }
    if (n < L) out[n++] = 1;                     // EOS, only where there is room
    n_out = n;
    status[b] = s_flags;
  }
  __syncthreads();
  for (int q = n_out + tid; q < L; q += LB_THREADS) out[q] = -100;
}

extern "C" int mrmt3_label_rows_fwd(const double* note_times, const int* note_meta, int n_notes, int n_stems,
                                    const unsigned long long* keep, const long long* start_frame,
                                    const long long* n_frames, const long long* total_frames, const double* scale,
                                    const int* shift, int batch, int pitch_base, int velocity_base, int tie_token,
                                    int program_base, int drum_base, int max_shift_steps, int steps_per_second,
                                    int sample_rate, int hop, int event_length, int num_special_tokens,
                                    long long* targets, int* status, void* stream) {
  MR_CHECK_ARG(keep && start_frame && n_frames && total_frames && scale && shift && targets && status,
               "label_rows_fwd: null pointer");
  MR_CHECK_ARG(n_notes >= 0 && (n_notes == 0 || (note_times && note_meta)), "label_rows_fwd: null note table of %d notes",
               n_notes);
  MR_CHECK_ARG(n_stems >= 1 && n_stems <= LB_MAX_STEMS, "label_rows_fwd: n_stems must be in [1, %d], got %d", LB_MAX_STEMS,
               n_stems);
  MR_CHECK_ARG(batch > 0 && event_length > 0 && max_shift_steps > 0 && steps_per_second > 0,
               "label_rows_fwd: batch, event_length, max_shift_steps and steps_per_second must be > 0");
  MR_CHECK_ARG(sample_rate > 0 && hop > 0, "label_rows_fwd: sample_rate and hop must be > 0");
  MR_CHECK_ARG(pitch_base >= 0 && velocity_base >= 0 && tie_token >= 0 && program_base >= 0 && drum_base >= 0 &&
                   num_special_tokens >= 0,
               "label_rows_fwd: token bases and num_special_tokens must be >= 0");
  NOTETAB_CHECK_META("label_rows_fwd", "note_meta", note_meta);
  const LbCodec c = {pitch_base, velocity_base, tie_token, program_base, drum_base, max_shift_steps, steps_per_second,
                     event_length, num_special_tokens, (double)sample_rate / (double)hop};
  hipLaunchKernelGGL(label_rows_kernel, dim3((unsigned)batch), dim3(LB_THREADS), 0, (hipStream_t)stream, note_times,
                     (const int4*)note_meta, n_notes, keep, start_frame, n_frames, total_frames, scale, shift, batch, c,
                     targets, status);
  MR_CHECK_LAUNCH("label_rows_fwd");
  g_label_launches.hit();
  return MRMT3_OK;
}

extern "C" unsigned long long mrmt3_label_launches(int reset) { return g_label_launches.read(reset); }
