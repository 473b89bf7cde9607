// corpus_stats.hip - the caption analysis of the reference's test epoch (include/care_hip.h, "Test epoch"): how many of an
// epoch's captions are distinct, how many of the distinct ones no training caption equals, how many words they use and how
// long they are (misc/utils.py:390-419) - as integers that stay on the device - and the `score` field of a prediction
// (care_caption_model_score).  int / uint64 / double only: the same in both library variants; ordinary vector atomics on
// 32- and 64-bit integers, no floating-point atomics; plain vector stores throughout.
//
// A caption is a row of at most 64 tokens cut at the first EOS or PAD (to_sentence, misc/utils.py:117-137): ONE WAVE per
// caption, token j on lane j.  Its key is a position-weighted sum in uint64 with wrap-around,
//   key = (h(n, 64) + sum_j h(token_j, j)) & key_mask,   h(a, i) = fin(a + 0x9E3779B97F4A7C15 (i + 1)),  fin = splitmix64's finaliser
// (h = care_mix64 of csrc/care_common.h; care_amd/captions.py restates it in numpy, bit for bit): a commutative sum, so the
// order of the wave's reduction does not matter.  Two captions are equal when their lengths are and a ballot of `token differs` is empty.
// A key only says where to look: every hit in the epoch set and in the training bank is confirmed token by token, so the
// counts are exact, not exact up to collisions.
//
// Two launches per batch, in stream order.  (1) corpus_append_kernel writes the batch's cut captions into rows
// [cursor, cursor + rows) of the epoch store (tokens [capacity, 64], length, key); the host knows every batch's row count, so
// the cursor is a host integer.  (2) corpus_insert_kernel probes the open-addressing table (slots [capacity] of store row
// numbers, -1 = empty) from key & (capacity - 1) with wrap-around and publishes its row by a 32-bit atomicCAS.  A slot can only
// name a row of an EARLIER launch or of launch (1) of this batch, which has completed before (2) starts: a reader of a slot
// never sees a half-written row, and no fence is needed inside a launch.  Of equal captions exactly one wins a slot - which
// one is a race, and nothing depends on it: the totals count captions, not rows.
#include "caption_core.h"

namespace {

#define CST ((hipStream_t)stream)
constexpr int CS_T = 256;                 // threads of a workgroup: four captions, one per wave
constexpr int CS_MAXLEN = CARE_CORPUS_MAX_CAPTION;
constexpr int CS_WORDS = CARE_CORPUS_BITMAP_WORDS;
constexpr int CS_POP_T = 1024;
static_assert(CS_MAXLEN == CARE_CAPTION_MAXLEN, "a store row holds one caption of the core's width");

struct AppendArgs {
  care_caption_rows cap;
  int rows, cursor, eos, pad;
  care_epoch_set set;
  uint64_t* keys_out;
};

// one wave per caption: cut at the first EOS / PAD, the key, the whole 64-token store row (zeros behind the caption)
__global__ __launch_bounds__(CS_T) void corpus_append_kernel(AppendArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (CS_T / 64) + (threadIdx.x >> 6);
  if (r >= a.rows) return;   // (uniform over the wave)
  int L = care_caption_len(a.cap, r);
  if (L < 0) L = 0;
  int tok = 0;
  if (lane < L) tok = care_caption_token(a.cap, r, lane);
  const uint64_t stop = __ballot(lane < L && (tok == (a.eos & 0xFFFF) || tok == (a.pad & 0xFFFF)));
  const int n = stop ? (int)__builtin_ctzll(stop) : L;
  const uint64_t part = lane < n ? care_mix64((uint64_t)(unsigned)tok, (uint64_t)lane) : 0ull;
  const uint64_t key = (care_wave_sum_64(part) + care_mix64((uint64_t)n, 64ull)) & a.set.key_mask;
  const int64_t g = (int64_t)a.cursor + r;
  a.set.tokens[g * CS_MAXLEN + lane] = lane < n ? tok : 0;
  if (lane == 0) {
    a.set.length[g] = n;
    a.set.keys[g] = key;
    if (a.keys_out) a.keys_out[r] = key;
  }
}

struct InsertArgs {
  int rows, cursor;
  care_corpus_bank bank;
  care_epoch_set set;
};

__global__ __launch_bounds__(CS_T) void corpus_insert_kernel(InsertArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (CS_T / 64) + (threadIdx.x >> 6);
  if (r >= a.rows) return;   // (uniform over the wave, like every branch below)
  const care_epoch_set& st = a.set;
  const int g = a.cursor + r;
  const int n = st.length[g];
  const uint64_t key = st.keys[g];
  const int tok = lane < n ? st.tokens[(int64_t)g * CS_MAXLEN + lane] : -1;
  unsigned long long* tot = (unsigned long long*)st.totals;

  // the words of the caption; the empty caption's one word (''.split(' ') == ['']) is the n_empty count itself
  if (lane < n) atomicOr(st.bitmap + (tok >> 5), 1u << (tok & 31));
  if (lane == 0) {
    atomicAdd(tot + CARE_CORPUS_N_CAPTIONS, 1ull);
    atomicAdd(tot + CARE_CORPUS_LENGTH_SUM, (unsigned long long)(n > 0 ? n : 1));
    if (n == 0) atomicAdd(tot + CARE_CORPUS_N_EMPTY, 1ull);
  }

  // the epoch set: probe from the key's slot, with wrap-around; the first of its kind wins an empty slot
  const int mask = st.capacity - 1;
  int s = (int)(key & (uint64_t)mask);
  bool first = false, placed = false;
  for (int probe = 0; probe < st.capacity; ++probe) {
    int old = 0;
    if (lane == 0) old = atomicCAS(st.slots + s, -1, g);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old == -1) { first = placed = true; break; }
    if (old < 0 || old >= st.capacity) break;   // (a slot the host did not initialise: never dereferenced, counted below)
    const int on = st.length[old];
    const int otok = lane < on ? st.tokens[(int64_t)old * CS_MAXLEN + lane] : -1;
    if (on == n && __ballot(otok != tok) == 0ull) { placed = true; break; }   // an equal caption holds the slot: a duplicate
    s = (s + 1) & mask;
  }
  if (!placed) {   // (cannot happen while the slots start at -1 and the rows stay within the capacity: the host sees to both)
    if (lane == 0) atomicAdd(tot + CARE_CORPUS_N_OVERFLOW, 1ull);
    return;
  }
  if (!first) return;

  // the first of its kind this epoch: novel unless a training caption equals it - the run of equal keys, token by token
  const care_corpus_bank& bk = a.bank;
  bool found = false;
  for (int64_t i = care_lower_bound(bk.keys, 0, bk.n, key); i < bk.n && bk.keys[i] == key; ++i) {
    const int64_t b0 = bk.start[i];
    const int64_t bn = bk.start[i + 1] - b0;
    if (bn != (int64_t)n) continue;
    const int btok = lane < n ? bk.tokens[b0 + lane] : -1;
    if (__ballot(btok != tok) == 0ull) { found = true; break; }
  }
  if (lane == 0) {
    atomicAdd(tot + CARE_CORPUS_N_DISTINCT, 1ull);
    if (!found) atomicAdd(tot + CARE_CORPUS_N_NOVEL, 1ull);
  }
}

// one workgroup: the set bits of the vocabulary bitmap, plus the empty word when an empty caption was seen
__global__ __launch_bounds__(CS_POP_T) void corpus_totals_kernel(care_epoch_set st) {
  __shared__ int part[CS_POP_T / 64];
  const int tid = threadIdx.x;
  int c = 0;
  for (int w = tid; w < CS_WORDS; w += CS_POP_T) c += __popc(st.bitmap[w]);
  c = care_wave_sum_i(c);
  if ((tid & 63) == 0) part[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int q = 0; q < CS_POP_T / 64; ++q) s += part[q];
    st.totals[CARE_CORPUS_USAGE] = (uint64_t)s + (st.totals[CARE_CORPUS_N_EMPTY] != 0 ? 1ull : 0ull);
  }
}

// one wave per clip: the normalised score of the hypothesis care_beam_select names, the one care_beam_winner copies
__global__ __launch_bounds__(64) void caption_model_score_kernel(const int32_t* nfin, const float* fscore, const int32_t* flen, int cap,
                                                                 const double* len_pow, int n_pow, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = nfin ? nfin[b] : 1;
  if (n > cap) n = cap;
  if (n <= 0) {
    if (lane == 0) out[b] = 0.0;
    return;
  }
  const double key = care_beam_select(n, b, cap, fscore, flen, len_pow, n_pow).key;
  if (lane == 0) out[b] = -key;
}

inline int cs_check_set(const care_epoch_set* s) {
  if (!s) return CARE_EINVAL;
  if (!s->slots || !s->tokens || !s->length || !s->keys || !s->bitmap || !s->totals) return CARE_EINVAL;
  if (s->capacity < 1 || (s->capacity & (s->capacity - 1)) != 0) return CARE_ESHAPE;
  if (!(care_aligned8(s->keys) && care_aligned8(s->totals))) return CARE_EALIGN;
  return 0;
}

}  // namespace

extern "C" int care_corpus_insert(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, int rows, int cursor,
                                  int eos, int pad, const care_corpus_bank* bank, const care_epoch_set* set, uint64_t* keys_out,
                                  void* stream) {
  if (!tokens || !length || !bank || rows < 0 || cursor < 0) return CARE_EINVAL;
  if (const int rc = cs_check_set(set)) return rc;
  if (!bank->keys || !bank->start || !bank->tokens || bank->n < 0) return CARE_EINVAL;
  if (bank->key_mask != set->key_mask) return CARE_EINVAL;   // (the bank's keys were masked on the host: one mask for both)
  if (const int rc = care_caption_rows_check(ld, col0, width, CARE_ESHAPE)) return rc;
  if ((int64_t)cursor + rows > (int64_t)set->capacity) return CARE_ESHAPE;
  if (!(care_aligned8(bank->keys) && care_aligned8(bank->start) && care_aligned8(keys_out))) return CARE_EALIGN;
  if (rows == 0) return 0;
  const int blocks = (rows + CS_T / 64 - 1) / (CS_T / 64);
  AppendArgs ap;
  ap.cap = {tokens, ld, col0, width, length};
  ap.rows = rows; ap.cursor = cursor; ap.eos = eos; ap.pad = pad;
  ap.set = *set;
  ap.keys_out = keys_out;
  hipLaunchKernelGGL(corpus_append_kernel, dim3(blocks), dim3(CS_T), 0, CST, ap);
  if (const int rc = care_launch_status()) return rc;
  InsertArgs in;
  in.rows = rows; in.cursor = cursor;
  in.bank = *bank;
  in.set = *set;
  hipLaunchKernelGGL(corpus_insert_kernel, dim3(blocks), dim3(CS_T), 0, CST, in);
  return care_launch_status();
}

extern "C" int care_corpus_totals(const care_epoch_set* set, void* stream) {
  if (const int rc = cs_check_set(set)) return rc;
  hipLaunchKernelGGL(corpus_totals_kernel, dim3(1), dim3(CS_POP_T), 0, CST, *set);
  return care_launch_status();
}

extern "C" int care_caption_model_score(const int32_t* nfin, const float* fscore, const int32_t* flen, int B, int cap,
                                        const double* len_pow, int n_pow, double* out, void* stream) {
  if (!fscore || !flen || !len_pow || !out || B < 0) return CARE_EINVAL;
  if (cap < 1 || cap > 64 || n_pow < 1) return CARE_EINVAL;
  if (!(care_aligned8(len_pow) && care_aligned8(out))) return CARE_EALIGN;
  if (B == 0) return 0;
  hipLaunchKernelGGL(caption_model_score_kernel, dim3(B), dim3(64), 0, CST, nfin, fscore, flen, cap, len_pow, n_pow, out);
  return care_launch_status();
}
