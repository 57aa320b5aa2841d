// Host-side planner of the grouped optimizer step (mrmt3_opt_ranges_plan): plain C++, no HIP — csrc/optim.hip alone includes it,
// and a CPU build with a main() of its own can too (a sanitizer run of the planner needs no GPU).
//
// The caller describes the trainable part of the flat parameter buffer as sorted, disjoint element ranges, each with its own
// weight decay and learning-rate factor.  The kernels see the ranges laid end to end as ONE virtual array of 16-byte groups
// (4 floats): record r says where range r starts in the buffer (begin4, in groups) and in the virtual array (start, the
// prefix sum of the lengths before it).  Record n_ranges is a sentinel whose `start` is the total — the kernels' loop bound.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mrmt3_hip.h"

struct MrOptRec {          // 32 bytes, the device table's record
  long long begin4;        // first 16-byte group of the range in the flat buffer
  long long start;         // 16-byte groups of the ranges before this one
  float wd, lr_scale;
  long long end4;          // one past the range's last group
};
static_assert(sizeof(MrOptRec) == 32, "device table record");

#define MR_OPT_MAX_RANGES 4096

// "" when the ranges are acceptable, else what is wrong with them (static text + the offending index in *bad)
static inline const char* mr_opt_ranges_problem(const mrmt3_opt_range* r, int n_ranges, size_t n, int* bad) {
  long long prev_end = 0;
  for (int i = 0; i < n_ranges; ++i) {
    *bad = i;
    if (r[i].begin < 0 || r[i].end < 0) return "negative bound";
    if ((r[i].begin & 3) != 0 || (r[i].end & 3) != 0) return "bounds must be multiples of 4 elements";
    if (r[i].end <= r[i].begin) return "empty or reversed range";
    if (r[i].begin < prev_end) return "ranges must be sorted and disjoint";
    if ((unsigned long long)r[i].end > (unsigned long long)n) return "range ends past the buffer";
    if (!(r[i].weight_decay >= 0.f) || !(r[i].weight_decay <= 3.4e38f)) return "weight_decay must be finite and >= 0";
    if (!(r[i].lr_scale >= 0.f) || !(r[i].lr_scale <= 3.4e38f)) return "lr_scale must be finite and >= 0";
    prev_end = r[i].end;
  }
  return "";
}

// fills n_ranges + 1 records; returns the number of trainable elements
static inline size_t mr_opt_ranges_fill(const mrmt3_opt_range* r, int n_ranges, MrOptRec* out) {
  long long start = 0;
  for (int i = 0; i < n_ranges; ++i) {
    out[i].begin4 = r[i].begin / 4;
    out[i].end4 = r[i].end / 4;
    out[i].start = start;
    out[i].wd = r[i].weight_decay;
    out[i].lr_scale = r[i].lr_scale;
    start += out[i].end4 - out[i].begin4;
  }
  out[n_ranges].begin4 = out[n_ranges].end4 = 0;
  out[n_ranges].start = start;
  out[n_ranges].wd = out[n_ranges].lr_scale = 0.f;
  return (size_t)start * 4;
}
