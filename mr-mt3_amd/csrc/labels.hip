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
// mrmt3_label_rows_parts_fwd builds the row of a virtual track: up to LB_MAX_PARTS parts, each a range of
// one note arena with its own stem mask, speed factor, transposition and delay.  The two scans run part after part, the
// successor of a note is looked for inside its own part, S_last, the bitmap and the event list are the row's; a 256-entry
// owner map in LDS tells when two parts keep the same (program, is_drum), which the trim cannot serve.  From the sort on
// both kernels run the same code.
//
// Integer and f64 work only, one rounding per operation (no fused multiply-add), ordinary vector stores.
#include "notetab.h"

#pragma clang fp contract(off)

#define LB_THREADS 256
#define LB_CAP 2048                              // ABI constant: events of one row's window, and tie-section entries
#define LB_TIE_WORDS 512                         // 128 programs x 128 pitches, one bit each
#define LB_MAX_STEMS 64
#define LB_MAX_PARTS 4                           // ABI constant: parts of one row of mrmt3_label_rows_parts_fwd
#define LB_OWNERS 256                            // (program, is_drum) pairs

#define LB_ST_EVENTS 1
#define LB_ST_TIES 2
#define LB_ST_ORDER 4
#define LB_ST_RANGE 8
#define LB_ST_SHARED 16

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

// A row's LDS: the event keys, the tie bitmap and its list, the counters
struct LbShared {
  unsigned long long k_time[LB_CAP], k_ord[LB_CAP];
  unsigned tie_bits[LB_TIE_WORDS];
  unsigned short tie_list[LB_CAP];
  int cnt[LB_THREADS];
  long long s_last;
  int n_ev, n_tie, n_out, s_flags;
};

// Note i of the table as row (mask, scale, shift) sees it.  flags: LB_ST_* raised by this note.  DELAYED: the table is a
// part of a virtual track, `delay` seconds (>= 0, 0: none) are added to every time after the scaling.
template <bool DELAYED>
__device__ __forceinline__ LbNote lb_note(const double* __restrict__ times, const int4* __restrict__ meta, int n_notes, int i,
                                          unsigned long long mask, double scale, int shift, double delay, int& flags) {
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
  if (DELAYED && delay != 0.0) {
    n.start = __dadd_rn(n.start, delay);
    n.end = __dadd_rn(n.end, delay);
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
    if (shift != 0) sj = __dmul_rn(sj, scale);
    if (DELAYED && delay != 0.0) sj = __dadd_rn(sj, delay);
    // the links order a group by (unscaled start, index); scaled or delayed starts may tie where those did not
    if ((shift != 0 || (DELAYED && delay != 0.0)) && (sj < n.start || (sj == n.start && j < i))) flags |= LB_ST_ORDER;
    if (n.end > sj) n.end = sj;
  }
  n.live = n.start < n.end;
  return n;
}

// One live note's events and tie bit into the row's LDS.  `ord`: the order key without the on bit and the velocity bin.
__device__ __forceinline__ void lb_collect(LbShared& sh, const LbNote& n, unsigned long long ord, long long lo, long long hi,
                                           long long bound, int sps) {
  const long long s_on = lb_step(n.start, sps);
  if (s_on >= lo && s_on < hi) {
    const int slot = atomicAdd(&sh.n_ev, 1);
    if (slot < LB_CAP) {
      sh.k_time[slot] = lb_time_key(n.start);
      sh.k_ord[slot] = ord | (1ull << 63) | (unsigned long long)n.vbin;
    }
  }
  if (!n.drum) {
    const long long s_off = lb_step(n.end, sps);
    // a key's events alternate on, off, on, ...: its last event before `bound` is this note's on event iff
    if (s_on < bound && s_off >= bound) atomicOr(&sh.tie_bits[(n.program << 2) | (n.pitch >> 5)], 1u << (n.pitch & 31));
    if (s_off >= lo && s_off < hi) {
      const int slot = atomicAdd(&sh.n_ev, 1);
      if (slot < LB_CAP) {
        sh.k_time[slot] = lb_time_key(n.end);
        sh.k_ord[slot] = ord;
      }
    }
  }
}

// From the collected events and the tie bitmap to the row: sort, compact, walk, fill.  Called by every thread after the
// barrier that follows the second scan.  VB: the bits of an on event's key that hold the velocity bin.
template <int VB>
__device__ __forceinline__ void lb_finish(LbShared& sh, const LbCodec& c, long long lo, long long* __restrict__ out,
                                          int* __restrict__ status, int tid) {
  const int events = sh.n_ev < LB_CAP ? sh.n_ev : LB_CAP;
  if (tid == 0 && sh.n_ev > LB_CAP) sh.s_flags |= LB_ST_EVENTS;

  // bitonic sort of the events on (time, order), padded with the largest key to a power of two
  int m = 1;
  while (m < events) m <<= 1;
  for (int q = events + tid; q < m; q += LB_THREADS) sh.k_time[q] = sh.k_ord[q] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < m; q += LB_THREADS) {
        const int l = q ^ j;
        if (l > q) {
          const unsigned long long tq = sh.k_time[q], tl = sh.k_time[l], oq = sh.k_ord[q], ol = sh.k_ord[l];
          const bool gt = tq > tl || (tq == tl && oq > ol);
          if (gt == ((q & k) == 0)) {
            sh.k_time[q] = tl; sh.k_time[l] = tq;
            sh.k_ord[q] = ol; sh.k_ord[l] = oq;
          }
        }
      }
      __syncthreads();
    }
  }

  // the bitmap -> the ordered list of (program, pitch) pairs: thread t owns words 2t and 2t + 1
  {
    const unsigned w0 = sh.tie_bits[2 * tid], w1 = sh.tie_bits[2 * tid + 1];
    sh.cnt[tid] = __popc(w0) + __popc(w1);
    __syncthreads();
    int at = 0;
    for (int q = 0; q < tid; ++q) at += sh.cnt[q];
    if (tid == LB_THREADS - 1) sh.n_tie = at + sh.cnt[tid];
    for (int h = 0; h < 2; ++h) {
      unsigned w = h ? w1 : w0;
      while (w) {
        const int bit = __ffs(w) - 1;
        w &= w - 1;
        if (at < LB_CAP) sh.tie_list[at] = (unsigned short)(((2 * tid + h) << 5) | bit);   // = program << 7 | pitch
        ++at;
      }
    }
  }
  __syncthreads();

  // the walk
  const int L = c.event_length;
  if (tid == 0) {
    int n = 0, cur_program = -1, cur_velocity = -1;
    const int ties = sh.n_tie < LB_CAP ? sh.n_tie : LB_CAP;
    if (sh.n_tie > LB_CAP) sh.s_flags |= LB_ST_TIES;
    for (int t = 0; t < ties && n < L; ++t) {
      const int program = sh.tie_list[t] >> 7, pitch = sh.tie_list[t] & 127;
      if (program != cur_program) {
        out[n++] = c.program_base + program + c.special;
        cur_program = program;
      }
      if (n < L) out[n++] = c.pitch_base + pitch + c.special;
    }
    if (n < L) out[n++] = c.tie_token + c.special;
    long long flushed = 0;
    for (int e = 0; e < events && n < L; ++e) {
      const unsigned long long o = sh.k_ord[e];
      const int on = (int)(o >> 63), drum = (int)(o >> 62) & 1, program = (int)(o >> 54) & 0xff,
                pitch = (int)(o >> 46) & 0xff, vbin = on ? (int)(o & ((1ull << VB) - 1)) : 0;
      const long long total = lb_step(lb_key_time(sh.k_time[e]), c.sps) - lo;
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
    sh.n_out = n;
    *status = sh.s_flags;
  }
  __syncthreads();
  for (int q = sh.n_out + tid; q < L; q += LB_THREADS) out[q] = -100;
}

__global__ __launch_bounds__(LB_THREADS) void label_rows_kernel(
    const double* __restrict__ times, const int4* __restrict__ meta, int n_notes, const unsigned long long* __restrict__ keep,
    const long long* __restrict__ start_frame, const long long* __restrict__ n_frames,
    const long long* __restrict__ total_frames, const double* __restrict__ scale_b, const int* __restrict__ shift_b,
    int batch, LbCodec c, long long* __restrict__ targets, int* __restrict__ status) {
  __shared__ LbShared sh;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= batch) return;
  const unsigned long long mask = keep[b];
  const double scale = scale_b[b];
  const int shift = shift_b[b];
  const long long f0 = start_frame[b], f1 = f0 + n_frames[b];
  const long long lo = lb_first_step(f0, c.fps, c.sps);
  const long long hi = f1 < total_frames[b] ? lb_first_step(f1, c.fps, c.sps) : 0x7fffffffffffffffLL;

  for (int q = tid; q < LB_TIE_WORDS; q += LB_THREADS) sh.tie_bits[q] = 0u;
  if (tid == 0) {
    sh.s_last = -0x7fffffffffffffffLL;
    sh.n_ev = 0;
    sh.s_flags = 0;
  }
  __syncthreads();

  // scan 1: the step of the subset's last event
  int flags = 0;
  long long last = -0x7fffffffffffffffLL;
  for (int i = tid; i < n_notes; i += LB_THREADS) {
    const LbNote n = lb_note<false>(times, meta, n_notes, i, mask, scale, shift, 0.0, flags);
    if (!n.live) continue;
    const long long s = lb_step(n.drum ? n.start : n.end, c.sps);      // (start < end: the off event is the later one)
    last = s > last ? s : last;
  }
  atomicMax(&sh.s_last, last);
  __syncthreads();
  const bool any = sh.s_last != -0x7fffffffffffffffLL;
  const long long bound = lo < sh.s_last ? lo : sh.s_last;

  // scan 2: the tie section's pairs and the window's events
  for (int i = tid; any && i < n_notes; i += LB_THREADS) {
    const LbNote n = lb_note<false>(times, meta, n_notes, i, mask, scale, shift, 0.0, flags);
    if (!n.live) continue;
    const unsigned long long ord = ((unsigned long long)n.drum << 62) | ((unsigned long long)n.program << 54) |
                                   ((unsigned long long)n.pitch << 46) | ((unsigned long long)(unsigned)i << 14);
    lb_collect(sh, n, ord, lo, hi, bound, c.sps);
  }
  if (flags) atomicOr(&sh.s_flags, flags);
  __syncthreads();
  lb_finish<14>(sh, c, lo, targets + (size_t)b * c.event_length, status + b, tid);
}

// A part of a row: a range of the arena, clamped into it whatever the arrays hold
struct LbPart {
  const double* times;
  const int4* meta;
  int count, shift;
  unsigned long long mask;
  double scale, delay;
};

__device__ __forceinline__ LbPart lb_part(const double* __restrict__ times, const int4* __restrict__ meta, int n_notes,
                                          const int* __restrict__ note_first, const int* __restrict__ note_count,
                                          const unsigned long long* __restrict__ keep,
                                          const long long* __restrict__ delay_frames, const double* __restrict__ scale,
                                          const int* __restrict__ shift, size_t at, double fps) {
  LbPart p;
  int first = note_first[at], count = note_count[at];
  if (first < 0 || first > n_notes) first = 0, count = 0;
  count = count < 0 ? 0 : (count > n_notes - first ? n_notes - first : count);
  p.mask = keep[at];
  if (p.mask == 0ull) count = 0;
  p.count = count;
  p.times = times + 2 * (size_t)first;
  p.meta = meta + first;
  p.shift = shift[at];
  p.scale = scale[at];
  const long long d = delay_frames[at];
  p.delay = d > 0 ? __ddiv_rn((double)d, fps) : 0.0;
  return p;
}

__global__ __launch_bounds__(LB_THREADS) void label_rows_parts_kernel(
    const double* __restrict__ times, const int4* __restrict__ meta, int n_notes, int n_parts,
    const int* __restrict__ note_first, const int* __restrict__ note_count, const unsigned long long* __restrict__ keep,
    const long long* __restrict__ delay_frames, const double* __restrict__ scale_b, const int* __restrict__ shift_b,
    const long long* __restrict__ start_frame, const long long* __restrict__ n_frames,
    const long long* __restrict__ total_frames, int batch, LbCodec c, long long* __restrict__ targets,
    int* __restrict__ status) {
  __shared__ LbShared sh;
  int* owner = sh.cnt;                           // the owner map lives where the compaction counts later (scan 1 only)
  static_assert(LB_OWNERS <= LB_THREADS, "the owner map borrows LbShared::cnt");
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= batch) return;
  const long long f0 = start_frame[b], f1 = f0 + n_frames[b];
  const long long lo = lb_first_step(f0, c.fps, c.sps);
  const long long hi = f1 < total_frames[b] ? lb_first_step(f1, c.fps, c.sps) : 0x7fffffffffffffffLL;

  for (int q = tid; q < LB_TIE_WORDS; q += LB_THREADS) sh.tie_bits[q] = 0u;
  for (int q = tid; q < LB_OWNERS; q += LB_THREADS) owner[q] = -1;
  if (tid == 0) {
    sh.s_last = -0x7fffffffffffffffLL;
    sh.n_ev = 0;
    sh.s_flags = 0;
  }
  __syncthreads();

  // scan 1: the step of the row's last event, and who keeps which (program, is_drum)
  int flags = 0;
  long long last = -0x7fffffffffffffffLL;
  for (int p = 0; p < n_parts; ++p) {
    const LbPart pt = lb_part(times, meta, n_notes, note_first, note_count, keep, delay_frames, scale_b, shift_b,
                              (size_t)b * n_parts + p, c.fps);
    for (int i = tid; i < pt.count; i += LB_THREADS) {
      const int z = pt.meta[i].z;
      if ((pt.mask >> ((z >> 16) & 63)) & 1ull) {
        const int key = (z & 0x7f) | ((z >> 1) & 0x80);                // program (a program above 127 is LB_ST_RANGE) | drum << 7
        const int old = atomicCAS(&owner[key], -1, p);
        if (old != -1 && old != p) flags |= LB_ST_SHARED;
      }
      const LbNote n = lb_note<true>(pt.times, pt.meta, pt.count, i, pt.mask, pt.scale, pt.shift, pt.delay, flags);
      if (!n.live) continue;
      const long long s = lb_step(n.drum ? n.start : n.end, c.sps);
      last = s > last ? s : last;
    }
  }
  atomicMax(&sh.s_last, last);
  __syncthreads();
  const bool any = sh.s_last != -0x7fffffffffffffffLL;
  const long long bound = lo < sh.s_last ? lo : sh.s_last;

  // scan 2: the tie section's pairs and the window's events; in the key the part comes before the index in the part
  for (int p = 0; any && p < n_parts; ++p) {
    const LbPart pt = lb_part(times, meta, n_notes, note_first, note_count, keep, delay_frames, scale_b, shift_b,
                              (size_t)b * n_parts + p, c.fps);
    for (int i = tid; i < pt.count; i += LB_THREADS) {
      const LbNote n = lb_note<true>(pt.times, pt.meta, pt.count, i, pt.mask, pt.scale, pt.shift, pt.delay, flags);
      if (!n.live) continue;
      const unsigned long long ord = ((unsigned long long)n.drum << 62) | ((unsigned long long)n.program << 54) |
                                     ((unsigned long long)n.pitch << 46) | ((unsigned long long)p << 44) |
                                     ((unsigned long long)(unsigned)i << 12);
      lb_collect(sh, n, ord, lo, hi, bound, c.sps);
    }
  }
  if (flags) atomicOr(&sh.s_flags, flags);
  __syncthreads();
  lb_finish<12>(sh, c, lo, targets + (size_t)b * c.event_length, status + b, tid);
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

extern "C" int mrmt3_label_rows_parts_fwd(const double* note_times, const int* note_meta, int n_notes, int n_parts,
                                          const int* note_first, const int* note_count, const unsigned long long* keep,
                                          const long long* delay_frames, const double* scale, const int* shift,
                                          const long long* start_frame, const long long* n_frames,
                                          const long long* total_frames, int batch, int pitch_base, int velocity_base,
                                          int tie_token, int program_base, int drum_base, int max_shift_steps,
                                          int steps_per_second, int sample_rate, int hop, int event_length,
                                          int num_special_tokens, long long* targets, int* status, void* stream) {
  MR_CHECK_ARG(note_first && note_count && keep && delay_frames && scale && shift && start_frame && n_frames &&
                   total_frames && targets && status,
               "label_rows_parts_fwd: null pointer");
  MR_CHECK_ARG(n_notes >= 0 && (n_notes == 0 || (note_times && note_meta)),
               "label_rows_parts_fwd: null note arena of %d notes", n_notes);
  MR_CHECK_ARG(n_parts >= 1 && n_parts <= LB_MAX_PARTS, "label_rows_parts_fwd: n_parts must be in [1, %d], got %d",
               LB_MAX_PARTS, n_parts);
  MR_CHECK_ARG(batch > 0 && event_length > 0 && max_shift_steps > 0 && steps_per_second > 0,
               "label_rows_parts_fwd: batch, event_length, max_shift_steps and steps_per_second must be > 0");
  MR_CHECK_ARG(sample_rate > 0 && hop > 0, "label_rows_parts_fwd: sample_rate and hop must be > 0");
  MR_CHECK_ARG(pitch_base >= 0 && velocity_base >= 0 && tie_token >= 0 && program_base >= 0 && drum_base >= 0 &&
                   num_special_tokens >= 0,
               "label_rows_parts_fwd: token bases and num_special_tokens must be >= 0");
  NOTETAB_CHECK_META("label_rows_parts_fwd", "note_meta", note_meta);
  const LbCodec c = {pitch_base, velocity_base, tie_token, program_base, drum_base, max_shift_steps, steps_per_second,
                     event_length, num_special_tokens, (double)sample_rate / (double)hop};
  hipLaunchKernelGGL(label_rows_parts_kernel, dim3((unsigned)batch), dim3(LB_THREADS), 0, (hipStream_t)stream, note_times,
                     (const int4*)note_meta, n_notes, n_parts, note_first, note_count, keep, delay_frames, scale, shift,
                     start_frame, n_frames, total_frames, batch, c, targets, status);
  MR_CHECK_LAUNCH("label_rows_parts_fwd");
  g_label_launches.hit();
  return MRMT3_OK;
}

extern "C" unsigned long long mrmt3_label_launches(int reset) { return g_label_launches.read(reset); }
