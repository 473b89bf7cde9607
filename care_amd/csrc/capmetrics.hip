// capmetrics.hip - the validation metrics over token ids (include/care_hip.h, "Validation metrics"): per decoded caption the
// sufficient statistics of corpus BLEU and its ROUGE-L (care_caption_stats), their sum over an epoch in a totals block that
// stays on the device (care_caption_totals), and the caption a beam search returns first (care_beam_winner).  int / fp32 /
// double in both library variants; no floating-point atomics; a row's bits depend on the row alone (the rules of reward.hip).
// The keys, the search, the ordered sums and the winner's order are csrc/caption_core.h's.
//
// The statistics: one workgroup of four waves per candidate.  The candidate's n-grams are the core's uint64 keys, the ones
// CIDEr is scored on (16 bits a token, in LDS); the clipped counts come from the video's clip table - sorted unique keys with
// the largest count over the video's references - by binary search, as integers.  The longest common subsequence is the
// bit-parallel recurrence on ONE 64-bit word: lane j holds candidate token j, and per reference token t (uniform over the wave)
//   M = ballot(cand[j] == t),  U = V & M,  V = (V + U) | (V & ~M),  V = ~0 at the start;
// the LCS is the number of zero bits among the low L bits.  A ballot and four 64-bit integer operations per reference token, no
// table, references of any length.  The waves take the video's references in turn; maxima of exact quotients and of integers
// do not depend on that order.
#include "caption_core.h"

// (a handful of double operations per row: each one rounded on its own, in both libraries)
#pragma clang fp contract(off)

namespace {

#define CST ((hipStream_t)stream)
constexpr int CT = 256;          // threads of a statistics workgroup (4 waves)
constexpr int CM_REC = 12;       // ints of a record
constexpr int TT = 1024;         // threads of the totals workgroup (16 waves)
constexpr double BETA2 = 1.2 * 1.2;

struct StatsArgs {
  care_caption_rows cap;
  const int32_t* video;
  int with_eos, eos;
  care_metric_bank bank;
  int32_t* rec; double* rouge;
};

__device__ __forceinline__ void cm_invalid_row(const StatsArgs& a, int r, int tid) {
  if (tid < CM_REC) a.rec[(int64_t)r * CM_REC + tid] = 0;
  if (tid == 0) a.rouge[r] = 0.0;
}

__global__ __launch_bounds__(CT) void caption_stats_kernel(StatsArgs a) {
  __shared__ uint64_t keys[CT];   // the candidate's n-grams: order 1 first, then 2, 3, 4, each in caption order
  __shared__ int clipc[CT];       // min(count in the candidate, clip table) at a key's FIRST occurrence, 0 elsewhere
  __shared__ int tok[CARE_CAPTION_MAXLEN];
  __shared__ int correct[4];
  __shared__ int w_lcs[4], w_dist[4], w_len[4];
  __shared__ double w_rec[4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const care_metric_bank& bk = a.bank;
  int L = care_caption_len(a.cap, r);
  const int v = a.video[r];
  if (L <= 0 || v < 0 || v >= bk.cider.n_videos) {   // (uniform over the workgroup, like every exit below)
    cm_invalid_row(a, r, tid);
    return;
  }
  const int rb = bk.cider.vid_start[v], re = bk.cider.vid_start[v + 1];
  if (re <= rb) {
    cm_invalid_row(a, r, tid);
    return;
  }
  if (tid < L) tok[tid] = care_caption_token(a.cap, r, tid);
  __syncthreads();
  if (!a.with_eos && tok[L - 1] == (a.eos & 0xFFFF)) L -= 1;   // (L == 0 from here on: a legitimate empty caption)

  // ---- BLEU: the clipped counts of the four orders (order n, 0-based, owns the keys [base[n], base[n + 1]))
  int base[5], ord, lo, hi;
  care_ngram_keys(tok, L, keys, base, ord, lo, hi);
  int c = 0;
  if (ord >= 0) {
    const uint64_t k = keys[tid];
    bool first;
    const int tf = care_ngram_tf(keys, lo, hi, k, first);
    if (first) {
      const int64_t cs = bk.clip_start[v], ce = bk.clip_start[v + 1];
      const int64_t i = care_lower_bound(bk.clip_keys, cs, ce, k);
      if (i < ce && bk.clip_keys[i] == k) {
        const int m = bk.clip_max[i];
        c = tf < m ? tf : m;
      }
    }
  }
  clipc[tid] = c;
  __syncthreads();
  if (tid < 4) {
    int s = 0;
    for (int j = base[tid]; j < base[tid + 1]; ++j) s += clipc[j];
    correct[tid] = s;
  }

  // ---- the closest reference length and ROUGE-L: the video's references dealt to the waves round-robin
  const int cand = lane < L ? tok[lane] : -1;   // (-1 equals no reference token)
  const uint64_t low = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
  int best_lcs = 0, best_dist = 0x7FFFFFFF, best_len = 0x7FFFFFFF;
  double best_rec = 0.0;
  for (int ref = rb + wave; ref < re; ref += 4) {   // (uniform over the wave)
    const int64_t ts = bk.ref_tok_start[ref], te = bk.ref_tok_start[ref + 1];
    const int rl = (int)(te - ts);
    const int d = rl > L ? rl - L : L - rl;
    if (d < best_dist || (d == best_dist && rl < best_len)) { best_dist = d; best_len = rl; }
    if (L > 0 && rl > 0) {
      uint64_t V = ~0ull;
      for (int64_t t0 = ts; t0 < te; t0 += 64) {
        const int n = te - t0 < 64 ? (int)(te - t0) : 64;
        const int mine = lane < n ? (bk.ref_tok[t0 + lane] & 0xFFFF) : -2;   // 64 reference tokens, one a lane
        for (int q = 0; q < n; ++q) {
          const int t = __builtin_amdgcn_readlane(mine, q);
          const uint64_t M = __ballot(cand == t);
          const uint64_t U = V & M;
          V = (V + U) | (V & ~M);
        }
      }
      const int lcs = __popcll(~V & low);
      if (lcs > best_lcs) best_lcs = lcs;
      const double rec = (double)lcs / (double)rl;
      if (rec > best_rec) best_rec = rec;
    }
  }
  if (lane == 0) { w_lcs[wave] = best_lcs; w_dist[wave] = best_dist; w_len[wave] = best_len; w_rec[wave] = best_rec; }
  __syncthreads();
  if (tid == 0) {
    int lcs = w_lcs[0], dist = w_dist[0], len = w_len[0];
    double rec = w_rec[0];
    for (int q = 1; q < 4; ++q) {
      if (w_lcs[q] > lcs) lcs = w_lcs[q];
      if (w_rec[q] > rec) rec = w_rec[q];
      if (w_dist[q] < dist || (w_dist[q] == dist && w_len[q] < len)) { dist = w_dist[q]; len = w_len[q]; }
    }
    int32_t* o = a.rec + (int64_t)r * CM_REC;
    o[0] = 1;
    o[1] = L;
    o[2] = len;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      o[3 + n] = L - n > 0 ? L - n : 0;
      o[7 + n] = correct[n];
    }
    o[11] = 0;
    double score = 0.0;
    if (L > 0 && lcs > 0) {
      const double prec = (double)lcs / (double)L;
      if (prec != 0.0 && rec != 0.0) score = ((1.0 + BETA2) * prec * rec) / (rec + BETA2 * prec);
    }
    a.rouge[r] = score;
  }
}

// one workgroup; thread t owns the rows t, t + 1024, ...; the doubles by a scan in lane order, then the waves in wave order
__global__ __launch_bounds__(TT) void caption_totals_kernel(const int32_t* rec, const double* rouge, const float* cider, int rows,
                                                            int64_t* tot_i, double* tot_d) {
  __shared__ long long si[16][CM_REC];
  __shared__ double sd[16][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long ai[CM_REC];
#pragma unroll
  for (int k = 0; k < CM_REC; ++k) ai[k] = 0;
  double ar = 0.0, ac = 0.0;
  for (int r = tid; r < rows; r += TT) {
    const int32_t* q = rec + (int64_t)r * CM_REC;
    if (q[0] != 0) {
      ai[0] += 1;
#pragma unroll
      for (int k = 2; k < CM_REC; ++k) ai[k] += q[k - 1];   // testlen, reflen, guess 1..4, correct 1..4
      ar += rouge[r];
      if (cider) ac += (double)cider[r];
    } else {
      ai[1] += 1;
    }
  }
#pragma unroll
  for (int k = 0; k < CM_REC; ++k) ai[k] = care_wave_sum_64(ai[k]);
  ar = care_wave_scan_total(ar);
  ac = care_wave_scan_total(ac);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < CM_REC; ++k) si[wave][k] = ai[k];
    sd[wave][0] = ar;
    sd[wave][1] = ac;
  }
  __syncthreads();
  if (tid < CM_REC) {
    long long s = 0;
    for (int q = 0; q < 16; ++q) s += si[q][tid];
    tot_i[tid] += s;
  }
  if (tid == 64 || tid == 65) {
    const int k = tid - 64;
    double s = sd[0][k];
    for (int q = 1; q < 16; ++q) s += sd[q][k];
    tot_d[k] += s;
  }
}

// one wave per clip: the tokens of the hypothesis care_beam_select names - the best normalised score, the earliest among equals
__global__ __launch_bounds__(64) void beam_winner_kernel(const int32_t* nfin, const float* fscore, const int32_t* flen,
                                                         const int32_t* fhyp, int cap, int w, const double* len_pow, int n_pow,
                                                         int32_t* tokens, int32_t* length) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = nfin[b];
  if (n > cap) n = cap;
  int32_t* out = tokens + (int64_t)b * w;
  if (n <= 0) {
    for (int j = lane; j < w; j += 64) out[j] = 0;
    if (lane == 0) length[b] = 0;
    return;
  }
  const int idx = care_beam_select(n, b, cap, fscore, flen, len_pow, n_pow).idx;
  int wl = flen[(int64_t)b * cap + idx];
  if (wl < 0) wl = 0;
  if (wl > w) wl = w;
  const int32_t* src = fhyp + ((int64_t)b * cap + idx) * w;
  for (int j = lane; j < w; j += 64) out[j] = j < wl ? src[j] : 0;
  if (lane == 0) length[b] = wl;
}

}  // namespace

extern "C" int care_caption_stats(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, const int32_t* video,
                                  int rows, int with_eos, int eos, const care_metric_bank* bank, int32_t* rec, double* rouge,
                                  void* stream) {
  if (!tokens || !length || !video || !rec || !rouge || !bank || rows < 0) return CARE_EINVAL;
  const care_cider_bank& cb = bank->cider;
  if (!cb.vid_start || cb.n_videos < 1 || cb.n_refs < 0 || !bank->clip_keys || !bank->clip_max || !bank->clip_start ||
      !bank->ref_tok || !bank->ref_tok_start)
    return CARE_EINVAL;
  if (const int rc = care_caption_rows_check(ld, col0, width, CARE_EINVAL)) return rc;
  if (!(care_aligned8(bank->clip_keys) && care_aligned8(bank->clip_start) && care_aligned8(bank->ref_tok_start) && care_aligned8(rouge)))
    return CARE_EALIGN;
  if (rows == 0) return 0;
  StatsArgs a;
  a.cap = {tokens, ld, col0, width, length};
  a.video = video;
  a.with_eos = with_eos; a.eos = eos;
  a.bank = *bank;
  a.rec = rec; a.rouge = rouge;
  hipLaunchKernelGGL(caption_stats_kernel, dim3(rows), dim3(CT), 0, CST, a);
  return care_launch_status();
}

extern "C" int care_caption_totals(const int32_t* rec, const double* rouge, const float* cider, int rows, int64_t* totals_i,
                                   double* totals_d, void* stream) {
  if (!rec || !rouge || !totals_i || !totals_d || rows < 0) return CARE_EINVAL;
  if (!(care_aligned8(rouge) && care_aligned8(totals_i) && care_aligned8(totals_d))) return CARE_EALIGN;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(caption_totals_kernel, dim3(1), dim3(TT), 0, CST, rec, rouge, cider, rows, totals_i, totals_d);
  return care_launch_status();
}

extern "C" int care_beam_winner(const int32_t* nfin, const float* fscore, const int32_t* flen, const int32_t* fhyp, int B, int cap,
                                int w, const double* len_pow, int n_pow, int32_t* tokens, int32_t* length, void* stream) {
  if (!nfin || !fscore || !flen || !fhyp || !len_pow || !tokens || !length || B < 0) return CARE_EINVAL;
  if (cap < 1 || cap > 64 || w < 1 || n_pow < 1) return CARE_EINVAL;
  if (!care_aligned8(len_pow)) return CARE_EALIGN;
  if (B == 0) return 0;
  hipLaunchKernelGGL(beam_winner_kernel, dim3(B), dim3(64), 0, CST, nfin, fscore, flen, fhyp, cap, w, len_pow, n_pow, tokens, length);
  return care_launch_status();
}
