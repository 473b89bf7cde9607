// reward.hip - self-critical sequence training (include/care_hip.h, "Self-critical sequence training"): the CIDEr-D of sampled
// captions over token ids (care_cider_score), advantages against a baseline (care_reward_advantage) and the advantage-weighted
// log-likelihood of the teacher-forced samples, forward and backward (care_reward_loss_fwd / _bwd).  fp32 / double in both
// library variants.
//
// The reward: one workgroup of four waves per candidate caption.  A caption has at most 64 tokens, so at most 250 n-grams
// (64 + 63 + 62 + 61) of orders 1..4, each ONE uint64 key (csrc/caption_core.h builds them, for care_caption_stats too): keys,
// weights and first-occurrence flags live in LDS (4 KB), only the bank - the corpus' keys with ln df, the references' sorted
// keys and weights - is read from memory, by binary search.  Every sum is in double and in one order (the norms in key order,
// a reference's terms by the core's scan in lane order, a wave's references in bank order, the waves in wave order): a row's
// bits depend on the row alone.  No atomics.
//
// The loss: the row sweeps of csrc/vocab_row.h, which the language loss runs too, with a plain maximum as the visitor - a live
// row is read once in the forward (in registers while V <= 12288) and once in the backward - and the weight of a row is its
// sequence's advantage over the number of live positions, which stays on the device.
#include "vocab_row.h"
#include "caption_core.h"

// the advantage has the bits of torch's elementwise fp32 operations: nothing is fused (vocab_row.h and caption_core.h, above
// this line, hold nothing that could be)
#pragma clang fp contract(off)

namespace {

#define RST ((hipStream_t)stream)
constexpr int RT = CARE_ROW_THREADS;   // threads of a workgroup (4 waves)

struct CiderArgs {
  care_caption_rows cap;
  const int32_t* video;
  int with_eos, eos;
  care_cider_bank bank;
  float* out;
};

__global__ __launch_bounds__(RT) void cider_score_kernel(CiderArgs a) {
  __shared__ uint64_t keys[RT];   // the candidate's n-grams: order 1 first, then 2, 3, 4, each in caption order
  __shared__ double wh[RT];       // tf (ln N - ln df) at a key's FIRST occurrence, 0 at its repeats and beyond the last key
  __shared__ int tok[CARE_CAPTION_MAXLEN];
  __shared__ double normh[4];
  __shared__ double part[4][4];   // [wave][order]
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const care_cider_bank& bk = a.bank;
  int L = care_caption_len(a.cap, r);
  const int v = a.video[r];
  if (L <= 0 || v < 0 || v >= bk.n_videos) {   // (uniform over the workgroup, like every exit below)
    if (tid == 0) a.out[r] = 0.f;
    return;
  }
  if (tid < L) tok[tid] = care_caption_token(a.cap, r, tid);
  __syncthreads();
  if (!a.with_eos && tok[L - 1] == (a.eos & 0xFFFF)) L -= 1;
  const int rb = bk.vid_start[v], re = bk.vid_start[v + 1];
  if (L <= 0 || re <= rb) {
    if (tid == 0) a.out[r] = 0.f;
    return;
  }
  int base[5], ord, lo, hi;
  care_ngram_keys(tok, L, keys, base, ord, lo, hi);
  const int K = base[4];   // <= 250
  double w = 0.0;
  if (ord >= 0) {
    const uint64_t k = keys[tid];
    bool first;
    const int tf = care_ngram_tf(keys, lo, hi, k, first);
    if (first) {
      const int64_t i = care_lower_bound(bk.corpus_keys, 0, bk.n_corpus, k);
      const double lndf = (i < bk.n_corpus && bk.corpus_keys[i] == k) ? bk.corpus_lndf[i] : 0.0;   // absent: df = 0
      w = (double)tf * (bk.ln_n - lndf);
    }
  }
  wh[tid] = w;
  __syncthreads();
  if (tid < 4) {
    double s = 0.0;
    for (int j = base[tid]; j < base[tid + 1]; ++j) s += wh[j] * wh[j];
    normh[tid] = sqrt(s);
  }
  __syncthreads();

  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  for (int ref = rb + wave; ref < re; ref += 4) {   // (uniform over the wave)
    const int64_t ks = bk.ref_start[ref], ke = bk.ref_start[ref + 1];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int i = lane; i < K; i += 64) {
      const double wi = wh[i];
      if (wi > 0.0) {   // a first occurrence with a weight: the others add exactly 0
        const uint64_t k = keys[i];
        const int64_t j = care_lower_bound(bk.ref_keys, ks, ke, k);
        if (j < ke && bk.ref_keys[j] == k) {
          const double wr = bk.ref_w[j];
          const double t = fmin(wi, wr) * wr;
          if (i < base[1]) s0 += t;
          else if (i < base[2]) s1 += t;
          else if (i < base[3]) s2 += t;
          else s3 += t;
        }
      }
    }
    const double dl = (double)(L - bk.ref_len[ref]);
    const double pen = exp(-(dl * dl) / 72.0);
    const double* nr = bk.ref_norm + (int64_t)ref * 4;
#define CID_ORDER(S, ACC, N)                                        \
  {                                                                 \
    double t = care_wave_scan_total(S);                               \
    const double nh_ = normh[N], nr_ = nr[N];                       \
    if (nh_ != 0.0 && nr_ != 0.0) t /= (nh_ * nr_);                 \
    ACC += t * pen;                                                 \
  }
    CID_ORDER(s0, acc0, 0) CID_ORDER(s1, acc1, 1) CID_ORDER(s2, acc2, 2) CID_ORDER(s3, acc3, 3)
#undef CID_ORDER
  }
  if (lane == 0) { part[wave][0] = acc0; part[wave][1] = acc1; part[wave][2] = acc2; part[wave][3] = acc3; }
  __syncthreads();
  if (tid == 0) {
    const double nref = (double)(re - rb);
    double tot = 0.0;
    for (int n = 0; n < 4; ++n) {
      double sn = part[0][n];
      for (int q = 1; q < 4; ++q) sn += part[q][n];
      tot += sn / nref;
    }
    a.out[r] = (float)(10.0 * (tot / 4.0));
  }
}

// *bad = rows whose video lies outside the bank (one workgroup, integers)
__global__ __launch_bounds__(RT) void cider_bad_kernel(const int32_t* video, int rows, int n_videos, int32_t* bad) {
  __shared__ int si[4];
  int c = 0;
  for (int r = threadIdx.x; r < rows; r += RT) {
    const int v = video[r];
    c += (v < 0 || v >= n_videos) ? 1 : 0;
  }
  c = care_wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) *bad = (si[0] + si[1]) + (si[2] + si[3]);
}

// one workgroup; thread t owns the clips t, t + 256, ...
__global__ __launch_bounds__(RT) void reward_advantage_kernel(const float* reward, const float* baseline, int B, int n, float* adv,
                                                              double* stats) {
  __shared__ double sr[RT], sb[RT];
  const int tid = threadIdx.x;
  double ar = 0.0, ab = 0.0;
  for (int b = tid; b < B; b += RT) {
    const float* r = reward + (int64_t)b * n;
    float* d = adv + (int64_t)b * n;
    if (baseline) {
      const float bl = baseline[b];
      for (int j = 0; j < n; ++j) {
        const float rj = r[j];
        d[j] = __fsub_rn(rj, bl);
        ar += (double)rj;
        ab += (double)bl;
      }
    } else {
      float s = r[0];
      for (int j = 1; j < n; ++j) s = __fadd_rn(s, r[j]);
      const float den = (float)(n - 1);
      for (int j = 0; j < n; ++j) {
        const float rj = r[j];
        const float base = __fdiv_rn(__fsub_rn(s, rj), den);
        d[j] = __fsub_rn(rj, base);
        ar += (double)rj;
        ab += (double)base;
      }
    }
  }
  sr[tid] = ar;
  sb[tid] = ab;
  __syncthreads();
  if (tid == 0) {
    double tr = sr[0], tb = sb[0];
    for (int q = 1; q < RT; ++q) { tr += sr[q]; tb += sb[q]; }
    const double cnt = (double)B * (double)n;
    stats[0] = tr / cnt;
    stats[1] = tb / cnt;
  }
}

// ------------------------------------------------------------------ the weighted log-likelihood
// forward of one row per workgroup.  NV4 > 0: the row's float4s live in registers (V <= 1024 NV4); NV4 == 0: the re-reading
// form for any V.
template <int NV4>
__global__ __launch_bounds__(RT) void reward_loss_fwd_kernel(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq,
                                                             int V, const int32_t* labels, float* rmax, float* lsum, float* logp) {
  __shared__ float sm[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int y = labels[r];
  if (y <= 0 || y >= V) {   // PAD or a label outside [0, V): not read
    if (tid == 0) { rmax[r] = 0.f; lsum[r] = 0.f; logp[r] = 0.f; }
    return;
  }
  const float* x = logits + (int64_t)(r / rows_per_seq) * seq_stride + (int64_t)(r % rows_per_seq) * ld;
  float best = -INFINITY;
  care_row<NV4> row;
  row.sweep(x, V, [&](float v, int) { best = v; },
            [&](const float4& q, int) { best = fmaxf(fmaxf(best, fmaxf(q.x, q.y)), fmaxf(q.z, q.w)); });
  best = care_block_max4(best, sm);
  const float s = care_block_sum4(row.sum_exp(best), sm);
  if (tid == 0) {
    const float ls = logf(s);
    rmax[r] = best;
    lsum[r] = ls;
    logp[r] = (x[y] - best) - ls;
  }
}

// the sums over rows in a fixed order (one workgroup): thread t adds rows t, t + 1024, ... in double, a scan in lane order,
// the waves in wave order.  A sequence whose advantage is exactly 0 adds nothing (its positions still count as live).
__global__ __launch_bounds__(1024) void reward_loss_reduce_kernel(const float* logp, const int32_t* labels, const float* adv, int V,
                                                                  int rows, int rows_per_seq, double* totals, float* loss,
                                                                  float* seq_logp, double* acc) {
  __shared__ double sa[16];
  __shared__ int sc[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a = 0.0;
  int c = 0;
  for (int r = tid; r < rows; r += 1024) {
    const int y = labels[r];
    if (y > 0 && y < V) {
      c += 1;
      const float ad = adv[r / rows_per_seq];
      if (ad != 0.f) a += (double)ad * (double)logp[r];
    }
  }
  a = care_wave_scan_total(a);
  c = care_wave_sum_i(c);
  if (lane == 0) { sa[wave] = a; sc[wave] = c; }
  __syncthreads();
  if (tid == 0) {
    a = sa[0]; c = sc[0];
    for (int q = 1; q < 16; ++q) { a += sa[q]; c += sc[q]; }
    const float l = c > 0 ? (float)(-(a / (double)c)) : 0.f;
    totals[0] = a;
    totals[1] = (double)c;
    *loss = l;
    if (acc) { acc[0] += (double)l; acc[1] += (double)c; }
  }
  if (seq_logp) {
    const int nseq = rows / rows_per_seq;
    for (int s = tid; s < nseq; s += 1024) {
      double t = 0.0;
      for (int j = 0; j < rows_per_seq; ++j) t += (double)logp[(int64_t)s * rows_per_seq + j];   // (0 on dead rows)
      seq_logp[s] = (float)t;
    }
  }
}

// backward: one workgroup per row of dlogits (sequence s, position p < seq_rows); live rows of a sequence with a non-zero
// advantage one read + one write, the others a zero fill (vocab_row.h: care_row_zero, care_row_map)
__global__ __launch_bounds__(RT) void reward_loss_bwd_kernel(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq,
                                                             int V, const int32_t* labels, const float* adv, const float* rmax,
                                                             const float* lsum, const double* totals, const float* g,
                                                             float* dlogits, int64_t ldd, int64_t dseq_stride, int seq_rows) {
  const int s = blockIdx.x / seq_rows, p = blockIdx.x % seq_rows;
  float* d = dlogits + (int64_t)s * dseq_stride + (int64_t)p * ldd;
  int y = 0, r = 0;
  float ad = 0.f;
  if (p < rows_per_seq) { r = s * rows_per_seq + p; y = labels[r]; ad = adv[s]; }
  const care_row_span sp = care_row_span_of(d, V);
  if (y <= 0 || y >= V || ad == 0.f) {
    care_row_zero(d, sp);
    return;
  }
  const float* x = logits + (int64_t)s * seq_stride + (int64_t)p * ld;
  const float m = rmax[r], ls = lsum[r];
  const float cf = (float)((double)(*g) * (double)ad / totals[1]);   // (a live row: n_live >= 1)
  care_row_map(x, d, sp, [=](float v, int c) { return cf * (expf((v - m) - ls) - (c == y ? 1.f : 0.f)); });
}

}  // namespace

extern "C" int care_cider_score(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, const int32_t* video,
                                int rows, int with_eos, int eos, const care_cider_bank* bank, float* out, int32_t* bad,
                                void* stream) {
  if (!tokens || !length || !video || !out || !bank || rows < 0) return CARE_EINVAL;
  if (!bank->corpus_keys || !bank->corpus_lndf || !bank->ref_keys || !bank->ref_w || !bank->ref_start || !bank->ref_norm ||
      !bank->ref_len || !bank->vid_start || bank->n_videos < 1 || bank->n_refs < 0 || bank->n_corpus < 0)
    return CARE_EINVAL;
  if (const int rc = care_caption_rows_check(ld, col0, width, CARE_EINVAL)) return rc;
  if (!(care_aligned8(bank->corpus_keys) && care_aligned8(bank->corpus_lndf) && care_aligned8(bank->ref_keys) &&
        care_aligned8(bank->ref_w) && care_aligned8(bank->ref_start) && care_aligned8(bank->ref_norm)))
    return CARE_EALIGN;
  if (rows == 0) return 0;
  CiderArgs a;
  a.cap = {tokens, ld, col0, width, length};
  a.video = video;
  a.with_eos = with_eos; a.eos = eos;
  a.bank = *bank;
  a.out = out;
  hipLaunchKernelGGL(cider_score_kernel, dim3(rows), dim3(RT), 0, RST, a);
  if (bad) hipLaunchKernelGGL(cider_bad_kernel, dim3(1), dim3(RT), 0, RST, video, rows, (int)bank->n_videos, bad);
  return care_launch_status();
}

extern "C" int care_reward_advantage(const float* reward, const float* baseline, int B, int n, float* adv, double* stats,
                                     void* stream) {
  if (!reward || !adv || !stats || B < 1 || n < 1 || (!baseline && n < 2)) return CARE_EINVAL;
  if (!care_aligned8(stats)) return CARE_EALIGN;
  hipLaunchKernelGGL(reward_advantage_kernel, dim3(1), dim3(RT), 0, RST, reward, baseline, B, n, adv, stats);
  return care_launch_status();
}

extern "C" int care_reward_loss_fwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V,
                                    const int32_t* labels, const float* adv, float* rmax, float* lsum, float* logp, double* totals,
                                    float* loss, float* seq_logp, double* acc, int rows, void* stream) {
  // (whole sequences only; without a rows_per_seq to divide by the call is CARE_EINVAL whatever stands here)
  const int bad = care_row_check_fwd(logits && labels && adv && rmax && lsum && logp && totals && loss, logits, ld, seq_stride,
                                     rows_per_seq, V, rows, rows_per_seq > 0 && rows % rows_per_seq == 0,
                                     care_aligned8(totals) && care_aligned8(acc));
  if (bad) return bad;
#define FWD_LAUNCH(N) hipLaunchKernelGGL(reward_loss_fwd_kernel<N>, dim3(rows), dim3(RT), 0, RST, logits, ld, seq_stride, rows_per_seq, V, labels, rmax, lsum, logp)
  if (V <= 4096) FWD_LAUNCH(4);
  else if (V <= 12288) FWD_LAUNCH(12);
  else FWD_LAUNCH(0);
#undef FWD_LAUNCH
  hipLaunchKernelGGL(reward_loss_reduce_kernel, dim3(1), dim3(1024), 0, RST, logp, labels, adv, V, rows, rows_per_seq, totals, loss,
                     seq_logp, acc);
  return care_launch_status();
}

extern "C" int care_reward_loss_bwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V,
                                    const int32_t* labels, const float* adv, const float* rmax, const float* lsum,
                                    const double* totals, const float* g, float* dlogits, int64_t ldd, int64_t dseq_stride,
                                    int seq_rows, int rows, void* stream) {
  unsigned grid = 0;
  const int bad = care_row_check_bwd(logits && labels && adv && rmax && lsum && totals && g && dlogits, logits, ld, seq_stride,
                                     rows_per_seq, V, dlogits, ldd, dseq_stride, seq_rows, rows, true, care_aligned8(totals), &grid);
  if (bad) return bad;
  hipLaunchKernelGGL(reward_loss_bwd_kernel, dim3(grid), dim3(RT), 0, RST, logits, ld, seq_stride, rows_per_seq, V, labels,
                     adv, rmax, lsum, totals, g, dlogits, ldd, dseq_stride, seq_rows);
  return care_launch_status();
}
