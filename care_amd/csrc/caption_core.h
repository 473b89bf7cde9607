// caption_core.h - what the caption kernels share, written once: CIDEr-D (reward.hip), BLEU / ROUGE-L and the beam winner
// (capmetrics.hip), the epoch's caption analysis and the `score` of a prediction (corpus_stats.hip), and the ordered sums
// of the concept metrics (concept_metrics.hip).  The rows of a caption batch and their host check; the uint64 n-gram keys
// of a candidate (CIDEr and BLEU score the SAME keys because this is the only code that builds them); the binary search
// over sorted keys; the wave sums - doubles in lane order, which is what "a row's bits depend on the row alone" rests on,
// and 64-bit integers; the order in which a beam's finished hypotheses are ranked.  The hash of the caption keys is
// care_mix64 of care_common.h.
//
// reward.hip, capmetrics.hip and concept_metrics.hip switch floating-point contraction off below their includes,
// corpus_stats.hip leaves it on, and all must get the same bits out of this file: NOTHING here may have the shape
// a * b + c, and no fp pragma belongs here (it would reach the includer's code).  Integers, compares, additions and one
// division only; the CIDEr and ROUGE arithmetic stays in its .hip file, below the pragma.
#pragma once
#include "care_common.h"

constexpr int CARE_CAPTION_MAXLEN = 64;   // tokens of a caption: token j on lane j, at most 250 n-grams of orders 1..4

// caption r = tokens[r * ld + col0 .. + min(length[r], width)): what care_cider_score, care_caption_stats and
// care_corpus_insert take first
struct care_caption_rows {
  const int32_t* tokens; int ld, col0, width;
  const int32_t* length;
};

// length[r] clamped to the width from above (a length <= 0 is the caller's to judge)
__device__ __forceinline__ int care_caption_len(const care_caption_rows& c, int r) {
  int L = c.length[r];
  if (L > c.width) L = c.width;
  return L;
}

// token j of caption r, as the 16 bits a key holds
__device__ __forceinline__ int care_caption_token(const care_caption_rows& c, int r, int j) {
  return c.tokens[(int64_t)r * c.ld + c.col0 + j] & 0xFFFF;
}

// 0, or the error of rows that do not fit; `too_wide` is what a width beyond the 64 tokens returns
static inline int care_caption_rows_check(int ld, int col0, int width, int too_wide) {
  if (width < 1 || col0 < 0) return CARE_EINVAL;
  if (width > CARE_CAPTION_MAXLEN) return too_wide;
  if ((int64_t)ld < (int64_t)col0 + width) return CARE_EINVAL;
  return 0;
}

// first index in [lo, hi) whose key is >= k (hi when none)
__device__ __forceinline__ int64_t care_lower_bound(const uint64_t* keys, int64_t lo, int64_t hi, uint64_t k) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the wave's sum by an inclusive scan in lane order (Hillis-Steele: lane l ends with v_0 + .. + v_l in ONE tree of additions),
// lane 63's total to every lane.  All 64 lanes must be active.
__device__ __forceinline__ double care_wave_scan_total(double v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return __shfl(v, 63, 64);
}

// the wave's sum of a 64-bit integer (long long, or uint64 with wrap-around), to every lane
template <class T>
__device__ __forceinline__ T care_wave_sum_64(T v) {
  static_assert(sizeof(T) == 8, "a 64-bit integer");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (T)__shfl_xor((long long)v, o, 64);
  return v;
}

// The n-grams of a candidate of L tokens (tok[] in LDS, 16 bits each) as uint64 keys in LDS: token j of an n-gram in bits
// [16 j, 16 j + 16), order 1 first, then 2, 3, 4, each in caption order.  Order n (0-based) owns the keys
// [base[n], base[n + 1]); thread t < base[4] owns key t, of order `ord`, in [lo, hi) (ord = -1, lo = hi = 0: none).  One
// workgroup of 256 threads, all of which call this: the keys are visible when it returns.  (base is a plain array on
// purpose: the callers index it by thread, and in a struct it would move from registers into LDS.)
__device__ __forceinline__ void care_ngram_keys(const int* tok, int L, uint64_t* keys, int (&base)[5], int& ord, int& lo, int& hi) {
  const int tid = threadIdx.x;
  base[0] = 0;
#pragma unroll
  for (int n = 0; n < 4; ++n) base[n + 1] = base[n] + (L - n > 0 ? L - n : 0);
  ord = -1;
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (tid >= base[n] && tid < base[n + 1]) ord = n;
  lo = 0;
  hi = 0;
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (ord == n) { lo = base[n]; hi = base[n + 1]; }
  if (ord >= 0) {
    const int pos = tid - lo;
    uint64_t k = 0;
    for (int j = 0; j <= ord; ++j) k |= (uint64_t)(unsigned)tok[pos + j] << (16 * j);
    keys[tid] = k;
  }
  __syncthreads();
}

// how often key k occurs among its order's keys [lo, hi), and whether the calling thread's is its first occurrence
__device__ __forceinline__ int care_ngram_tf(const uint64_t* keys, int lo, int hi, uint64_t k, bool& first_out) {
  const int tid = threadIdx.x;
  int tf = 0;
  bool first = true;
  for (int j = lo; j < hi; ++j)
    if (keys[j] == k) {
      tf += 1;
      if (j < tid) first = false;
    }
  first_out = first;
  return tf;
}

// The hypothesis a beam search returns first, by one wave: lane i < n holds finished hypothesis i of clip b (`cap` slots a
// clip), its key -score / length ** alpha (len_pow[length], the length clamped to [0, n_pow - 1]) - the key of a stable
// ascending sort, NaN behind everything, +inf on the empty lanes.  Every lane gets the winner's key and index: a finished one
// before an empty lane, a number before NaN, the smaller key, the lower index.  n >= 1.
struct care_beam_choice {
  double key;
  int idx;
};

__device__ __forceinline__ care_beam_choice care_beam_select(int n, int b, int cap, const float* fscore, const int32_t* flen,
                                                           const double* len_pow, int n_pow) {
  const int lane = threadIdx.x;
  double key = INFINITY;
  bool have = false;
  if (lane < n) {
    const int len = flen[(int64_t)b * cap + lane];
    const int li = len < 0 ? 0 : (len > n_pow - 1 ? n_pow - 1 : len);
    key = -((double)fscore[(int64_t)b * cap + lane] / len_pow[li]);
    have = true;
  }
  int idx = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ok = __shfl_xor(key, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    const int oh = __shfl_xor((int)have, o, 64);
    bool take;
    if (oh != (int)have) take = oh != 0;
    else if ((ok != ok) != (key != key)) take = key != key;
    else if (ok < key) take = true;
    else if (ok > key) take = false;
    else take = oi < idx;
    if (take) { key = ok; idx = oi; have = oh != 0; }
  }
  return {key, idx};
}
