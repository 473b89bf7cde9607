// consensus.hip - consensus (minimum-Bayes-risk) selection among a clip's own candidate captions (include/care_hip.h,
// "Consensus captions"): care_consensus_score gives every candidate the CIDEr-D it gets with the clip's OTHER candidates as
// its reference set - the keys, counts, weights, clipped cosine and length penalty of care_cider_score (csrc/reward.hip), from
// the same caption core - and names the candidate that agrees most with the rest.  fp32 / double in both library variants.
//
// One launch, one workgroup of four waves per clip, everything of the clip in LDS: per candidate a slab of 256 keys and 256
// weights (tf (ln N - ln df) at a key's first occurrence, 0 at its repeats and beyond its last key: what cider_score_kernel
// keeps for ONE candidate), its four norms, its tokens and its length - 4400 bytes a candidate, 137.5 KB at the 32 candidates
// the entry point takes.  Only ln df is read from memory (the bank's corpus table, by binary search), and the searches of all
// candidates run side by side: the keys of the clip are dealt to the threads as one list, not a candidate at a time.
// A wave takes a candidate j and walks the others in ascending i; a lane that owns a first-occurrence key of j scans i's keys
// of the same order (at most 64).  Every sum is in double and in one order - the norms in key order, a pair's terms by the
// core's scan in lane order, a candidate's references in ascending i - so a clip's bits depend on the clip alone.  No sort,
// no atomics.
#include "caption_core.h"

// the arithmetic of cider_score_kernel, bit for bit: nothing is fused (caption_core.h, above this line, holds nothing that
// could be)
#pragma clang fp contract(off)

namespace {

constexpr int CT = 256;     // threads of a workgroup (4 waves)
constexpr int SLAB = 256;   // keys / weights of a candidate (at most 250 are used)

struct ConsArgs {
  care_caption_rows cap;
  const int32_t* count;
  int n, with_eos, eos;
  const uint64_t* corpus_keys;
  const double* corpus_lndf;
  int64_t n_corpus;
  double ln_n;
  float* score;
  float* pairs;
  int32_t* winner;
  int32_t* winner_row;
};

// dynamic LDS of a clip of n candidates: keys, weights, norms, scores (8-byte entries), tokens, lengths, key offsets
constexpr int cons_lds_bytes(int n) { return n * (SLAB * 16 + 4 * 8 + 8 + CARE_CAPTION_MAXLEN * 4 + 4) + (n + 1) * 4 + 4; }

// the n-grams of order o (0-based) of a caption of L tokens: their number, and their place [lo, hi) among the caption's keys
__device__ __forceinline__ int cons_order_count(int L, int o) { return L - o > 0 ? L - o : 0; }
__device__ __forceinline__ void cons_order_range(int L, int o, int& lo, int& hi) {
  int s = 0;
  lo = 0;
  hi = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = cons_order_count(L, q);
    if (q == o) { lo = s; hi = s + c; }
    s += c;
  }
}

__global__ __launch_bounds__(CT) void consensus_kernel(ConsArgs a) {
  extern __shared__ __align__(16) unsigned char cons_lds[];
  const int n = a.n;
  uint64_t* keys = reinterpret_cast<uint64_t*>(cons_lds);   // [n][SLAB]: order 1 first, then 2, 3, 4, each in caption order
  double* wt = reinterpret_cast<double*>(keys + n * SLAB);  // [n][SLAB]
  double* norm = wt + n * SLAB;                             // [n][4]
  double* sc = norm + n * 4;                                // [n]: the scores
  int* tok = reinterpret_cast<int*>(sc + n);                // [n][64]
  int* len = tok + n * CARE_CAPTION_MAXLEN;                 // [n]: tokens after the EOS rule
  int* kstart = len + n;                                    // [n + 1]: candidate j owns the clip's keys [kstart[j], kstart[j + 1])
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = b * n;
  int m = a.count ? a.count[b] : n;
  m = m < 0 ? 0 : (m > n ? n : m);

  // ---- phase A: the slabs of the m valid candidates
  for (int e = tid; e < m * CARE_CAPTION_MAXLEN; e += CT) {
    const int j = e >> 6, c = e & 63;
    if (c < care_caption_len(a.cap, r0 + j)) tok[e] = care_caption_token(a.cap, r0 + j, c);
  }
  __syncthreads();
  if (tid < m) {
    int L = care_caption_len(a.cap, r0 + tid);
    if (L < 0) L = 0;
    if (!a.with_eos && L > 0 && tok[tid * CARE_CAPTION_MAXLEN + L - 1] == (a.eos & 0xFFFF)) L -= 1;
    len[tid] = L;
  }
  __syncthreads();
  if (tid <= m) {
    int s = 0;
    for (int q = 0; q < tid; ++q) {
      const int L = len[q];
#pragma unroll
      for (int o = 0; o < 4; ++o) s += cons_order_count(L, o);
    }
    kstart[tid] = s;
  }
  for (int j = 0; j < m; ++j) {   // (uniform over the workgroup: care_ngram_keys holds a barrier)
    uint64_t* kj = keys + j * SLAB;
    int base[5], ord, lo, hi;
    care_ngram_keys(tok + j * CARE_CAPTION_MAXLEN, len[j], kj, base, ord, lo, hi);
    double tf = 0.0;
    if (ord >= 0) {
      bool first;
      const int c = care_ngram_tf(kj, lo, hi, kj[tid], first);
      if (first) tf = (double)c;
    }
    wt[j * SLAB + tid] = tf;   // (the count for now; 0 at a repeat and beyond the last key)
  }
  __syncthreads();
  const int W = kstart[m];
  for (int e = tid; e < W; e += CT) {   // every first occurrence of the clip: its weight from the corpus table
    int j = 0;
    while (e >= kstart[j + 1]) ++j;
    const int at = j * SLAB + (e - kstart[j]);
    const double tf = wt[at];
    if (tf > 0.0) {
      const uint64_t k = keys[at];
      const int64_t i = care_lower_bound(a.corpus_keys, 0, a.n_corpus, k);
      const double lndf = (i < a.n_corpus && a.corpus_keys[i] == k) ? a.corpus_lndf[i] : 0.0;   // absent: df = 0
      wt[at] = tf * (a.ln_n - lndf);
    }
  }
  __syncthreads();
  if (tid < 4 * m) {
    const int j = tid >> 2;
    int lo, hi;
    cons_order_range(len[j], tid & 3, lo, hi);
    double s = 0.0;
    for (int x = lo; x < hi; ++x) s += wt[j * SLAB + x] * wt[j * SLAB + x];
    norm[tid] = sqrt(s);
  }
  __syncthreads();

  // ---- phase B: wave w scores the candidates w, w + 4, ... against the others in ascending i
  for (int j = wave; j < n; j += 4) {   // (uniform over the wave, like everything up to the lane loop)
    float* prow = a.pairs ? a.pairs + (int64_t)(r0 + j) * n : nullptr;
    if (j >= m) {
      if (lane == 0) a.score[r0 + j] = 0.f;
      if (prow)
        for (int i = lane; i < n; i += 64) prow[i] = 0.f;
      continue;
    }
    const int Lj = len[j];
    const int b1 = cons_order_count(Lj, 0), b2 = b1 + cons_order_count(Lj, 1), b3 = b2 + cons_order_count(Lj, 2),
              Kj = b3 + cons_order_count(Lj, 3);
    const uint64_t* kj = keys + j * SLAB;
    const double* wj = wt + j * SLAB;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    for (int i = 0; i < n; ++i) {
      if (i == j || i >= m) {
        if (prow && lane == 0) prow[i] = 0.f;
        continue;
      }
      const int Li = len[i];
      const uint64_t* ki = keys + i * SLAB;
      const double* wi = wt + i * SLAB;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      for (int x = lane; x < Kj; x += 64) {
        const double wh = wj[x];
        if (wh > 0.0) {   // a first occurrence with a weight: the others add exactly 0
          const uint64_t k = kj[x];
          const int o = (x >= b1 ? 1 : 0) + (x >= b2 ? 1 : 0) + (x >= b3 ? 1 : 0);
          int lo, hi;
          cons_order_range(Li, o, lo, hi);
          for (int y = lo; y < hi; ++y)
            if (ki[y] == k) {   // (the first match is the first occurrence: the one that holds the weight)
              const double wr = wi[y];
              const double t = fmin(wh, wr) * wr;
              if (o == 0) s0 += t;
              else if (o == 1) s1 += t;
              else if (o == 2) s2 += t;
              else s3 += t;
              break;
            }
        }
      }
      const double dl = (double)(Lj - Li);
      const double pen = exp(-(dl * dl) / 72.0);
      double t0, t1, t2, t3;
#define CONS_ORDER(S, T, ACC, N)                                    \
  {                                                                 \
    double t = care_wave_scan_total(S);                             \
    const double nh_ = norm[j * 4 + N], nr_ = norm[i * 4 + N];      \
    if (nh_ != 0.0 && nr_ != 0.0) t /= (nh_ * nr_);                 \
    T = t * pen;                                                    \
    ACC += T;                                                       \
  }
      CONS_ORDER(s0, t0, acc0, 0) CONS_ORDER(s1, t1, acc1, 1) CONS_ORDER(s2, t2, acc2, 2) CONS_ORDER(s3, t3, acc3, 3)
#undef CONS_ORDER
      if (prow && lane == 0) prow[i] = (float)(10.0 * ((((t0 + t1) + t2) + t3) / 4.0));
    }
    if (lane == 0) {
      double s = 0.0;
      if (m > 1) {
        const double den = (double)(m - 1);
        const double tot = ((acc0 / den + acc1 / den) + acc2 / den) + acc3 / den;
        s = 10.0 * (tot / 4.0);
      }
      sc[j] = s;
      a.score[r0 + j] = (float)s;
    }
  }
  __syncthreads();

  // ---- phase C: the largest score AS IT IS WRITTEN (the double rounded to fp32), the lower index among equals.  Not the
  // doubles themselves: two copies of one caption get the same terms in another order of i, their sums may differ in the last
  // bit of a double, and the winner among them would be decided by that bit instead of by the index.
  if (wave == 0) {
    float best = lane < m ? (float)sc[lane] : -INFINITY;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) {
      a.winner[b] = m > 0 ? bi : -1;
      if (a.winner_row) a.winner_row[b] = m > 0 ? r0 + bi : -1;
    }
  }
}

}  // namespace

extern "C" int care_consensus_score(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, const int32_t* count,
                                    int clips, int n, int with_eos, int eos, const care_cider_bank* bank, float* score, float* pairs,
                                    int32_t* winner, int32_t* winner_row, void* stream) {
  if (!tokens || !length || !bank || !score || !winner || clips < 0 || n < 1) return CARE_EINVAL;
  if (!bank->corpus_keys || !bank->corpus_lndf || bank->n_corpus < 0 || bank->n_videos < 1) return CARE_EINVAL;
  if (const int rc = care_caption_rows_check(ld, col0, width, CARE_ESHAPE)) return rc;
  if (n > CARE_CONSENSUS_MAX_N || (int64_t)clips * n > 0x7FFFFFFF) return CARE_ESHAPE;
  if (!(care_aligned8(bank->corpus_keys) && care_aligned8(bank->corpus_lndf))) return CARE_EALIGN;
  if (clips == 0) return 0;
  ConsArgs a;
  a.cap = {tokens, ld, col0, width, length};
  a.count = count;
  a.n = n; a.with_eos = with_eos; a.eos = eos;
  a.corpus_keys = bank->corpus_keys; a.corpus_lndf = bank->corpus_lndf; a.n_corpus = bank->n_corpus; a.ln_n = bank->ln_n;
  a.score = score; a.pairs = pairs; a.winner = winner; a.winner_row = winner_row;
  const int lds = cons_lds_bytes(n);
  static std::atomic<unsigned long long> ok{0};
  if (lds > 64 * 1024)   // (raised once a device, so to what the largest n needs)
    if (const int e = care_allow_dynamic_lds(reinterpret_cast<const void*>(&consensus_kernel), cons_lds_bytes(CARE_CONSENSUS_MAX_N), ok))
      return e;
  hipLaunchKernelGGL(consensus_kernel, dim3(clips), dim3(CT), lds, (hipStream_t)stream, a);
  return care_launch_status();
}
