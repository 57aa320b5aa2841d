// The MT3 event grammar: a per-row state machine whose allowed set is the next step's ban mask.  Its device
// code, the stand-alone mrmt3_grammar_* entry points, and the decoder's side of it: mrmt3_decoder_set_grammar /
// mrmt3_decoder_grammar_active and the launch of dec_grammar_step after the step's tail (decode_tail.hip).
#include "decode.h"

// A row's state: the scalars below and `active`, a 128 x 128 bit set over (program, pitch) — in the tie section the
// pairs declared so far, in the body the notes sounding.  Two copies per row: at token step t every row reads its
// parent's state from copy t & 1 and writes its own to copy (t + 1) & 1, so beam reparenting needs no ordering between
// rows.  One wave per row: lane l carries words 8 l .. 8 l + 7 of the set from the parent's copy to the row's own (the
// 2 KB copy is what reparenting costs), the lane that owns the touched word edits it on the way, and only the 128-bit
// slice of the program in force enters the mask.
#define GRAM_WORDS 512        // 128 * 128 / 32
#define GRAM_TIE 0
#define GRAM_BODY 1
#define GRAM_VEL_UNSET 0
#define GRAM_VEL_OFF 1
#define GRAM_VEL_ON 2
struct GramS { int mode, program, velocity, cur, acc; };     // program -1 = unset; cur, acc in steps
struct GramRow { GramS s; int _r[3]; unsigned active[GRAM_WORDS]; };   // 32 + 2048 bytes
struct GramHdr { int parity; int _r[3]; const uint8_t* carry; const uint8_t* ban; };   // stand-alone state: which copy is current
static_assert(sizeof(GramRow) == 32 + 4 * GRAM_WORDS && sizeof(GramHdr) == 32, "grammar state layout");
#define GRAM_OP_NONE 0
#define GRAM_OP_SET 1
#define GRAM_OP_CLEAR 2

// Push one token: the scalars change here, the bit operation on `active` (bit `idx`) is returned.  A token the
// grammar does not allow in this state changes nothing it should not: the masks keep such tokens from being emitted.
__device__ __forceinline__ int gram_push(const mrmt3_grammar& g, GramS& s, int tok, int& idx) {
  idx = 0;
  unsigned v = (unsigned)(tok - g.shift0);
  if (v < (unsigned)g.n_shift) {
    if (s.mode == GRAM_BODY) s.acc += (int)v;
    return GRAM_OP_NONE;
  }
  if (s.mode == GRAM_TIE) {
    if (tok == g.tie) s.mode = GRAM_BODY;
    else if ((v = (unsigned)(tok - g.program0)) < (unsigned)g.n_program) s.program = (int)v;
    else if ((v = (unsigned)(tok - g.pitch0)) < (unsigned)g.n_pitch && s.program >= 0) {
      idx = s.program * 128 + (int)v;
      return GRAM_OP_SET;
    }
    return GRAM_OP_NONE;
  }
  // any non-shift token in the body closes the shift run: decode_events restarts its step count there
  s.cur = max(s.cur, s.acc);
  s.acc = 0;
  if ((v = (unsigned)(tok - g.program0)) < (unsigned)g.n_program) s.program = (int)v;
  else if ((v = (unsigned)(tok - g.velocity0)) < (unsigned)g.n_velocity) s.velocity = v ? GRAM_VEL_ON : GRAM_VEL_OFF;
  else if ((v = (unsigned)(tok - g.pitch0)) < (unsigned)g.n_pitch && s.program >= 0 && s.velocity != GRAM_VEL_UNSET) {
    idx = s.program * 128 + (int)v;
    return s.velocity == GRAM_VEL_ON ? GRAM_OP_SET : GRAM_OP_CLEAR;
  }
  return GRAM_OP_NONE;
}

// Is token `col` allowed in state s?  act / car: the 128-bit slices of `active` / the carry for s.program (zeros when unset).
__device__ __forceinline__ bool gram_allowed(const mrmt3_grammar& g, const GramS& s, const unsigned (&act)[4],
                                             const unsigned (&car)[4], bool has_carry, int col) {
  const bool body = s.mode == GRAM_BODY;
  if (col == g.eos) return body;
  if (col == g.tie) return !body;
  unsigned v = (unsigned)(col - g.shift0);
  if (v < (unsigned)g.n_shift) return body && v >= 1u && s.cur < s.acc + (int)v && s.acc + (int)v <= g.max_shift_steps;
  if ((v = (unsigned)(col - g.pitch0)) < (unsigned)g.n_pitch) {
    if (s.program < 0) return false;
    unsigned aw = act[0], cw = car[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if ((v >> 5) == (unsigned)j) { aw = act[j]; cw = car[j]; }
    const bool on = (aw >> (v & 31u)) & 1u, carried = (cw >> (v & 31u)) & 1u;
    if (!body) return !on && (!has_carry || carried);
    return s.velocity == GRAM_VEL_ON || (s.velocity == GRAM_VEL_OFF && on);
  }
  if ((v = (unsigned)(col - g.velocity0)) < (unsigned)g.n_velocity) return body;
  if ((v = (unsigned)(col - g.program0)) < (unsigned)g.n_program) return true;
  if ((v = (unsigned)(col - g.drum0)) < (unsigned)g.n_drum) return body && s.velocity == GRAM_VEL_ON;
  return false;   // pad, unk, ids outside the codec
}

// mrow[c] = 1 where the row may not emit c next (not allowed, or banned by the static mask).  One wave.
__device__ __forceinline__ void gram_write_mask(const mrmt3_grammar& g, const GramS& s, const unsigned (&act)[4],
                                                const unsigned (&car)[4], bool has_carry,
                                                const uint8_t* __restrict__ sban, int V, uint8_t* __restrict__ mrow, int lane) {
  if ((V & 3) == 0) {       // rows of the mask are 4-byte aligned: one store per four columns
    for (int c = lane * 4; c < V; c += 256) {
      unsigned w = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool banned = !gram_allowed(g, s, act, car, has_carry, c + j) || (sban != nullptr && sban[c + j]);
        w |= (banned ? 1u : 0u) << (8 * j);
      }
      *(unsigned*)(mrow + c) = w;
    }
  } else {
    for (int c = lane; c < V; c += 64)
      mrow[c] = (!gram_allowed(g, s, act, car, has_carry, c) || (sban != nullptr && sban[c])) ? 1 : 0;
  }
}

// The 128-bit slice of a row's carry for `program` (zeros without a carry or a program).
__device__ __forceinline__ void gram_carry_slice(const uint8_t* __restrict__ carry_row, int program, unsigned (&car)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    car[j] = (carry_row != nullptr && program >= 0) ? ((const unsigned*)carry_row)[program * 4 + j] : 0u;
}

// One wave: `dst` = `src` (the parent's state) after `tok`, and the row's next mask.
__device__ __forceinline__ void gram_advance_row(const mrmt3_grammar& g, const GramRow* __restrict__ src,
                                                 GramRow* __restrict__ dst, const uint8_t* __restrict__ carry_row,
                                                 const uint8_t* __restrict__ sban, int tok, int V,
                                                 uint8_t* __restrict__ mrow, int lane) {
  const u32x4 lo = ((const u32x4*)src->active)[lane * 2], hi = ((const u32x4*)src->active)[lane * 2 + 1];
  unsigned a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  GramS s = src->s;
  int idx;
  const int op = gram_push(g, s, tok, idx);
  if (op != GRAM_OP_NONE && (idx >> 8) == lane) {        // word idx >> 5 lives in lane (idx >> 5) >> 3
    const unsigned bit = 1u << (idx & 31);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (((idx >> 5) & 7) == e) a[e] = op == GRAM_OP_SET ? (a[e] | bit) : (a[e] & ~bit);
  }
  u32x4 o0, o1;
  o0.x = a[0]; o0.y = a[1]; o0.z = a[2]; o0.w = a[3]; o1.x = a[4]; o1.y = a[5]; o1.z = a[6]; o1.w = a[7];
  ((u32x4*)dst->active)[lane * 2] = o0;
  ((u32x4*)dst->active)[lane * 2 + 1] = o1;
  if (lane == 0) dst->s = s;
  // the slice of the program now in force: words 4 p .. 4 p + 3 sit in lane p >> 1, upper or lower half
  unsigned act[4], car[4];
  const int p = max(s.program, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned mine = (p & 1) ? a[4 + j] : a[j];
    act[j] = s.program >= 0 ? (unsigned)__shfl((int)mine, p >> 1, 64) : 0u;
  }
  gram_carry_slice(carry_row, s.program, car);
  gram_write_mask(g, s, act, car, carry_row != nullptr, sban, V, mrow, lane);
}

// Start state of every row and its first mask.  One wave per row, 8 rows per workgroup.
__global__ __launch_bounds__(512) void gram_init_kernel(const mrmt3_grammar* __restrict__ gd, mrmt3_grammar gv, GramHdr* hdr,
                                                        GramRow* __restrict__ rows0, const uint8_t* __restrict__ carry,
                                                        const uint8_t* __restrict__ sban, int rows, int V,
                                                        uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (hdr != nullptr && blockIdx.x == 0 && threadIdx.x == 0) { hdr->parity = 0; hdr->carry = carry; hdr->ban = sban; }
  if (r >= rows) return;
  const mrmt3_grammar g = gd ? *gd : gv;
  const uint8_t* crow = carry ? carry + (size_t)r * MRMT3_GRAMMAR_SET_BYTES : nullptr;
  GramRow* dst = rows0 + r;
  // a row that starts in the body (no tie section) starts with what was sounding; one that starts in the tie section
  // declares its own set
  const bool seed = !g.tie_section && crow != nullptr;
  u32x4 z0 = {0u, 0u, 0u, 0u}, z1 = z0;
  if (seed) { z0 = ((const u32x4*)crow)[lane * 2]; z1 = ((const u32x4*)crow)[lane * 2 + 1]; }
  ((u32x4*)dst->active)[lane * 2] = z0;
  ((u32x4*)dst->active)[lane * 2 + 1] = z1;
  GramS s;
  s.mode = g.tie_section ? GRAM_TIE : GRAM_BODY; s.program = -1; s.velocity = GRAM_VEL_UNSET; s.cur = 0; s.acc = 0;
  if (lane == 0) dst->s = s;
  const unsigned none[4] = {0u, 0u, 0u, 0u};       // no program yet: no pitch is allowed, the slices do not matter
  gram_write_mask(g, s, none, none, crow != nullptr, sban, V, mask + (size_t)r * V, lane);
}

// The decoder's step kernel, after the tail: the tail has written step t's tokens (and, under beam search, parents) and
// advanced the step counter.
__global__ __launch_bounds__(512) void dec_grammar_step(const mrmt3_grammar* __restrict__ gd, char* __restrict__ blob,
                                                        int max_rows, const int64_t* __restrict__ tokens, int tok_ld,
                                                        const int* __restrict__ state, const int* __restrict__ bp, int rows,
                                                        int V, int pad, uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  const int p = state[ST_T] - 1, npre = state[ST_NPRE];      // the position the tail has just closed
  if (p + 1 <= npre || r >= rows) return;                    // a prefix step emitted nothing
  const int t = p - npre;
  const int tok = (int)tokens[(size_t)r * tok_ld + t + 1];
  if (tok == pad) return;                                    // the row (beam: its group) had finished before this step
  const mrmt3_grammar g = *gd;
  const GramHdr* hdr = (const GramHdr*)blob;                 // carry and static ban of this decode (mrmt3_decoder_set_grammar)
  GramRow* buf = (GramRow*)(blob + sizeof(GramHdr));
  const int parent = bp ? bp[((size_t)t * rows + r) * 2] : r;
  const GramRow* src = buf + (size_t)(t & 1) * max_rows + parent;
  GramRow* dst = buf + (size_t)((t + 1) & 1) * max_rows + r;
  gram_advance_row(g, src, dst, hdr->carry ? hdr->carry + (size_t)r * MRMT3_GRAMMAR_SET_BYTES : nullptr, hdr->ban, tok, V,
                   mask + (size_t)r * V, lane);
}

// The same on a caller's state (mrmt3_grammar_advance); gram_flip_kernel then makes the written copy current.
__global__ __launch_bounds__(512) void gram_advance_kernel(mrmt3_grammar g, char* __restrict__ blob,
                                                           const int32_t* __restrict__ parents,
                                                           const int64_t* __restrict__ tokens, int rows, int V, int pad,
                                                           uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const GramHdr* hdr = (const GramHdr*)blob;
  GramRow* buf = (GramRow*)(blob + sizeof(GramHdr));
  const int par = hdr->parity & 1;
  const int tok = (int)tokens[r];
  // a padded row keeps ITS state: carried over to the copy that becomes current, mask untouched
  const bool idle = tok == pad;
  const int parent = (parents && !idle && (unsigned)parents[r] < (unsigned)rows) ? parents[r] : r;
  const GramRow* src = buf + (size_t)par * rows + parent;
  GramRow* dst = buf + (size_t)(par ^ 1) * rows + r;
  if (idle) {
    ((u32x4*)dst->active)[lane * 2] = ((const u32x4*)src->active)[lane * 2];
    ((u32x4*)dst->active)[lane * 2 + 1] = ((const u32x4*)src->active)[lane * 2 + 1];
    if (lane == 0) dst->s = src->s;
    return;
  }
  gram_advance_row(g, src, dst, hdr->carry ? hdr->carry + (size_t)r * MRMT3_GRAMMAR_SET_BYTES : nullptr, hdr->ban, tok, V,
                   mask + (size_t)r * V, lane);
}
__global__ void gram_flip_kernel(GramHdr* hdr) { hdr->parity ^= 1; }

__global__ __launch_bounds__(512) void gram_active_kernel(const char* __restrict__ blob, int rows, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const GramHdr* hdr = (const GramHdr*)blob;
  const GramRow* src = (const GramRow*)(blob + sizeof(GramHdr)) + (size_t)(hdr->parity & 1) * rows + r;
  u32x4* o = (u32x4*)(out + (size_t)r * MRMT3_GRAMMAR_SET_BYTES);
  o[lane * 2] = ((const u32x4*)src->active)[lane * 2];
  o[lane * 2 + 1] = ((const u32x4*)src->active)[lane * 2 + 1];
}

// The `active` set a row's emitted tokens leave behind, pushed again from the start state (mrmt3_decoder_grammar_active):
// ids[r * ld + 1 ..] up to EOS, pad or `limit` tokens (*limit_dev - npre when limit < 0: the token steps run so far).
// One wave per row; the set lives in LDS and lane 0 walks the tokens.
__global__ __launch_bounds__(64) void gram_replay_kernel(const mrmt3_grammar* __restrict__ gd, mrmt3_grammar gv,
                                                         const int64_t* __restrict__ ids,
                                                         int ld, int limit, const int* __restrict__ state,
                                                         const uint8_t* __restrict__ carry, int carry_row_stride,
                                                         uint8_t* __restrict__ out) {
  __shared__ unsigned act[GRAM_WORDS];
  const int lane = threadIdx.x, r = blockIdx.x;
  const mrmt3_grammar g = gd ? *gd : gv;
  const unsigned* crow = carry ? (const unsigned*)(carry + (size_t)r * carry_row_stride * MRMT3_GRAMMAR_SET_BYTES) : nullptr;
  for (int w = lane; w < GRAM_WORDS; w += 64) act[w] = (!g.tie_section && crow) ? crow[w] : 0u;
  __syncthreads();
  if (lane == 0) {
    GramS s;
    s.mode = g.tie_section ? GRAM_TIE : GRAM_BODY; s.program = -1; s.velocity = GRAM_VEL_UNSET; s.cur = 0; s.acc = 0;
    const int n = limit >= 0 ? limit : state[ST_T] - state[ST_NPRE];
    for (int t = 0; t < n && t + 1 < ld; ++t) {
      const int tok = (int)ids[(size_t)r * ld + t + 1];
      if (tok == g.eos || tok == g.pad) break;
      int idx;
      const int op = gram_push(g, s, tok, idx);
      if (op == GRAM_OP_SET) act[idx >> 5] |= 1u << (idx & 31);
      else if (op == GRAM_OP_CLEAR) act[idx >> 5] &= ~(1u << (idx & 31));
    }
  }
  __syncthreads();
  unsigned* o = (unsigned*)(out + (size_t)r * MRMT3_GRAMMAR_SET_BYTES);
  for (int w = lane; w < GRAM_WORDS; w += 64) o[w] = act[w];
}

__global__ void gram_desc_set_kernel(mrmt3_grammar* rec, mrmt3_grammar v) { *rec = v; }

// ---- event grammar entry points --------------------------------------------------------------------------------
static int grammar_check(const char* who, const mrmt3_grammar* g, int V) {
  MR_CHECK_ARG(g != nullptr, "%s: null grammar", who);
  const int r[5][2] = {{g->shift0, g->n_shift}, {g->pitch0, g->n_pitch}, {g->velocity0, g->n_velocity},
                       {g->program0, g->n_program}, {g->drum0, g->n_drum}};
  for (int i = 0; i < 5; ++i)
    MR_CHECK_ARG(r[i][0] >= 0 && r[i][1] >= 1 && (long)r[i][0] + r[i][1] <= V, "%s: id range %d (%d + %d) outside the vocabulary %d",
                 who, i, r[i][0], r[i][1], V);
  MR_CHECK_ARG(g->n_pitch <= 128 && g->n_program <= 128, "%s: the state holds 128 x 128 (program, pitch) pairs", who);
  MR_CHECK_ARG(g->n_velocity >= 2, "%s: need an off and an on velocity", who);
  MR_CHECK_ARG(g->tie >= 0 && g->tie < V && g->eos >= 0 && g->eos < V && g->pad >= 0 && g->pad < V && g->eos != g->pad,
               "%s: tie / eos / pad ids outside the vocabulary %d", who, V);
  MR_CHECK_ARG(g->max_shift_steps >= 0, "%s: max_shift_steps < 0", who);
  return MRMT3_OK;
}

extern "C" size_t mrmt3_grammar_state_bytes(int rows) {
  return rows > 0 ? sizeof(GramHdr) + 2 * (size_t)rows * sizeof(GramRow) : 0;
}

extern "C" int mrmt3_grammar_init(const mrmt3_grammar* g, void* state, const uint8_t* carry, const uint8_t* banned_mask,
                                  int rows, int V, uint8_t* mask_out, void* stream) {
  MR_CHECK_ARG(state && mask_out && rows > 0 && V > 0, "grammar_init: bad args");
  MR_CHECK_ARG(((uintptr_t)state & 15) == 0, "grammar_init: state must be 16-byte aligned");
  int rc = grammar_check("grammar_init", g, V);
  if (rc != MRMT3_OK) return rc;
  hipLaunchKernelGGL(gram_init_kernel, dim3((unsigned)ceil_div(rows, 8)), dim3(512), 0, (hipStream_t)stream,
                     (const mrmt3_grammar*)nullptr, *g, (GramHdr*)state, (GramRow*)((char*)state + sizeof(GramHdr)), carry,
                     banned_mask, rows, V, mask_out);
  MR_CHECK_LAUNCH("grammar_init");
  return MRMT3_OK;
}

extern "C" int mrmt3_grammar_advance(const mrmt3_grammar* g, void* state, const int32_t* parents, const int64_t* tokens,
                                     int rows, int V, uint8_t* mask_out, void* stream) {
  MR_CHECK_ARG(state && tokens && mask_out && rows > 0 && V > 0, "grammar_advance: bad args");
  int rc = grammar_check("grammar_advance", g, V);
  if (rc != MRMT3_OK) return rc;
  hipLaunchKernelGGL(gram_advance_kernel, dim3((unsigned)ceil_div(rows, 8)), dim3(512), 0, (hipStream_t)stream, *g,
                     (char*)state, parents, tokens, rows, V, g->pad, mask_out);
  hipLaunchKernelGGL(gram_flip_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (GramHdr*)state);
  MR_CHECK_LAUNCH("grammar_advance");
  return MRMT3_OK;
}

extern "C" int mrmt3_grammar_active(const void* state, int rows, uint8_t* out, void* stream) {
  MR_CHECK_ARG(state && out && rows > 0, "grammar_active: bad args");
  hipLaunchKernelGGL(gram_active_kernel, dim3((unsigned)ceil_div(rows, 8)), dim3(512), 0, (hipStream_t)stream,
                     (const char*)state, rows, out);
  MR_CHECK_LAUNCH("grammar_active");
  return MRMT3_OK;
}

extern "C" int mrmt3_grammar_replay(const mrmt3_grammar* g, const int64_t* ids, int ld, int rows, int n_tokens, int V,
                                    const uint8_t* carry, uint8_t* out, void* stream) {
  MR_CHECK_ARG(ids && out && rows > 0 && ld >= 1 && n_tokens >= 0, "grammar_replay: bad args");
  int rc = grammar_check("grammar_replay", g, V);
  if (rc != MRMT3_OK) return rc;
  hipLaunchKernelGGL(gram_replay_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, (const mrmt3_grammar*)nullptr,
                     *g, ids, ld, n_tokens, (const int*)nullptr, carry, 1, out);
  MR_CHECK_LAUNCH("grammar_replay");
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_set_grammar(mrmt3_decoder* D, const mrmt3_grammar* g, const uint8_t* carry, void* stream) {
  MR_CHECK_ARG(D && D->tokens, "decoder_set_grammar: call decoder_begin first");
  mrmt3_decoder::Tail& T = D->tail;
  if (!g) {
    if (T.gram) { T.ban = D->gsban; T.gram = 0; T.ban_stride = 0; }
    return MRMT3_OK;
  }
  MR_CHECK_ARG(!T.gram, "decoder_set_grammar: already set for this decode");
  int rc = grammar_check("decoder_set_grammar", g, D->V);
  if (rc != MRMT3_OK) return rc;
  MR_CHECK_ARG(g->eos == D->eos && g->pad == D->pad, "decoder_set_grammar: eos / pad differ from decoder_begin's");
  if (!D->gblob) {
    hipError_t e = hipMalloc((void**)&D->gblob, mrmt3_grammar_state_bytes(D->maxB));
    if (e == hipSuccess) e = hipMalloc((void**)&D->gmask, (size_t)D->maxB * D->V);
    if (e == hipSuccess) e = hipMalloc((void**)&D->gdesc, sizeof(mrmt3_grammar));
    if (e != hipSuccess) {
      mrmt3_set_error("decoder_set_grammar: hipMalloc failed: %s", hipGetErrorString(e));
      return MRMT3_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(gram_desc_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, D->gdesc, *g);
  // the static mask in force (greedy: mrmt3_decoder_set_ban, beam: mrmt3_decoder_begin_beam) goes into the row masks
  hipLaunchKernelGGL(gram_init_kernel, dim3((unsigned)ceil_div(D->B, 8)), dim3(512), 0, (hipStream_t)stream,
                     (const mrmt3_grammar*)nullptr, *g, (GramHdr*)D->gblob, (GramRow*)(D->gblob + sizeof(GramHdr)), carry,
                     T.ban, D->B, D->V, D->gmask);
  MR_CHECK_LAUNCH("decoder_set_grammar");
  D->gcarry = carry; D->gsban = T.ban;
  T.ban = D->gmask; T.ban_stride = D->V; T.gram = 1;
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_grammar_active(mrmt3_decoder* D, uint8_t* out, void* stream) {
  MR_CHECK_ARG(D && out && D->tokens && D->tail.gram, "decoder_grammar_active: no constrained decode on the handle");
  const mrmt3_decoder::Tail& T = D->tail;
  if (T.k > 0) {
    MR_CHECK_ARG(D->beam_out, "decoder_grammar_active: call decoder_beam_finalize first");
    hipLaunchKernelGGL(gram_replay_kernel, dim3((unsigned)T.groups), dim3(64), 0, (hipStream_t)stream,
                       (const mrmt3_grammar*)D->gdesc, mrmt3_grammar{}, D->beam_out, D->beam_out_ld, D->beam_out_len,
                       (const int*)D->state,
                       D->gcarry, T.k, out);
  } else {
    hipLaunchKernelGGL(gram_replay_kernel, dim3((unsigned)D->B), dim3(64), 0, (hipStream_t)stream,
                       (const mrmt3_grammar*)D->gdesc, mrmt3_grammar{}, (const int64_t*)D->tokens, D->maxLen + 1, -1,
                       (const int*)D->state,
                       D->gcarry, 1, out);
  }
  MR_CHECK_LAUNCH("decoder_grammar_active");
  return MRMT3_OK;
}

void mrmt3_dec_launch_grammar_step(mrmt3_decoder* D, hipStream_t s) {
  hipLaunchKernelGGL(dec_grammar_step, dim3((unsigned)ceil_div(D->B, 8)), dim3(512), 0, s, (const mrmt3_grammar*)D->gdesc,
                     D->gblob, D->maxB, (const int64_t*)D->tokens, D->maxLen + 1, (const int*)D->state,
                     D->tail.k > 0 ? (const int*)D->tail.bp : (const int*)nullptr, D->B, D->V, D->pad, D->gmask);
}
