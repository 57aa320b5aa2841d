// What the decoder's translation units share (decode.hip: the handle, the per-layer kernels and the step launcher;
// decode_tail.hip: the greedy / sampled / beam tails; decode_grammar.hip: the event grammar): the sizes, the device state
// block, the handle and the host functions that cross files.  A kernel is launched only from the file that defines it.
#pragma once
#include "common.h"

#define DMODEL 512
#define DEC_MAXB 256

// state block: [0] step t, [1] all finished, [2] step at which the last row finished (-1), [4+b] finished[b]
#define ST_T 0
#define ST_ALL 1
#define ST_FIN 2
#define ST_NPRE 3   // number of prefix (memory) positions fed before the start token
#define ST_FLAGS 4
#define ST_CNT (ST_FLAGS + DEC_MAXB)   // workgroups of the current argmax launch that have finished

// a vocabulary row in one wave's registers (LOGP_REGS values per lane, V <= 64 * LOGP_REGS): rl[i] = column lane + 64 i
#define LOGP_REGS 32

// the sampled tail's device record (decode_tail.hip)
struct SampleCfg {
  float temperature;   // > 0; 1 leaves the logits' bits alone
  int top_k;           // 0 = off
  float top_p;         // 1 = off, else in (0, 1)
  unsigned key;        // the seed folded to 32 bits (sample_seed_key)
};

// The weights of mrmt3_decoder_weights by value: the caller's per-layer host arrays need not outlive mrmt3_decoder_begin.
// Pointers only (no padding): mrmt3_decoder_begin compares two tables byte by byte.
struct DecLayer {
  const void *ln_self, *w_qkv, *w_o_self, *ln_cross, *w_q_cross, *w_o_cross, *ln_ff, *w_wi, *w_wo;
};
struct DecWeights {
  const void* embed;
  const float* pos;
  const void* lm_head;
  const float* final_ln;
  DecLayer layer[64];   // entries past the handle's layer count stay null
};

struct mrmt3_decoder {
  int L, d, H, dff, V, maxB, maxLen, maxEnc, wdt, inner;
  float eps;
  void *kc, *vc;  // [L][maxB][maxLen][inner]
  float *x, *q, *o, *g, *logits;
  float* blp;     // beam search: [2][maxLen][maxB] f32 log-probabilities beside the backpointers (dec_beam_select)
  SampleCfg* samp;   // sampling parameters and seed, read by dec_sample at every step (mrmt3_decoder_set_sampling)
  int* state;
  // per-batch
  DecWeights w;
  const void* cross_kv;
  const float* prefix;   // [B][n_prefix][d] f32 memory rows fed before the start token (or null)
  int B, encLen, eos, pad, start;
  int64_t* tokens;
  // what the step's tail bakes into the graph: k = 0 greedy (ban = null: the plain argmax), k > 0 beam search.
  // The capture key is the struct's bytes (same()), so every field is part of it: a new one cannot be left out.
  struct Tail {
    const uint8_t* ban;
    float* logp;      // greedy: per-token log-probabilities [B][logp_ld] (null = off: the plain / banned argmax)
    float* bscore;
    int* bp;
    int* hyp;
    int k, groups;
    int ban_stride;   // 0: `ban` is one static [V] mask; V: the event grammar's mask per row (`gram`)
    int gram;         // 1: dec_grammar_step follows the tail (mrmt3_decoder_set_grammar)
    int logp_ld;
    int sample;       // 1: dec_sample draws the token (its parameters live in `samp`, not here: they may change per call)
    float length_penalty;
    int _fill;        // always 0: keeps the struct free of padding
    bool same(const Tail& o) const { return memcmp(this, &o, sizeof(Tail)) == 0; }
  } tail;
  static_assert(sizeof(Tail) == 5 * sizeof(void*) + 8 * sizeof(int), "Tail must have no padding: same() compares its bytes");
  Tail cap_tail;    // tail of the captured graph
  int n_prefix;     // set by mrmt3_decoder_set_prefix since the last begin
  hipGraph_t graph;
  hipGraphExec_t exec;
  int captured;     // 1 = exec valid for the current (B, encLen, pointers)
  int graph_failed;  // 1 = capture failed once; run with plain launches
  int captures;      // step graphs instantiated so far (mrmt3_decoder_capture_count)
  // event grammar (mrmt3_decoder_set_grammar), allocated on first use and kept: the step graph bakes the addresses in
  char* gblob;             // GramHdr + 2 x maxB GramRow
  uint8_t* gmask;          // [maxB][V]
  mrmt3_grammar* gdesc;    // the descriptor, read by the step at every replay
  const uint8_t* gcarry;   // this decode's carry (also in the blob's header)
  const uint8_t* gsban;    // the static mask that was in force when the grammar went on
  const int64_t* beam_out; // what the last mrmt3_decoder_beam_finalize wrote, for mrmt3_decoder_grammar_active
  int beam_out_ld, beam_out_len;
};

// the step's last kernel(s): greedy argmax (banned or not), the sampled tail, or the beam select + KV-cache reorder; then
// the grammar's step when it is on (decode_tail.hip)
void mrmt3_dec_launch_tail(mrmt3_decoder* D, hipStream_t s);
// dec_grammar_step after the tail (decode_grammar.hip)
void mrmt3_dec_launch_grammar_step(mrmt3_decoder* D, hipStream_t s);
