// loss.hip - the training criteria on the logits and the concept probabilities (include/care_hip.h, "Training criteria"):
// the label-smoothed language loss of misc/Crit/crit_lang.py:27-103 and the normalised BCE of misc/Crit/crit_attribute.py:38-48,
// forward and backward.  fp32 in both library variants.
//
// The [rows, V] logits are the largest tensor of a training step (512 clips x 29 x 10547 fp32 = 626 MB), so the forward reads
// a live row once (the row stays in registers between the max / arg-max / sum sweep and the sum of exponentials) and the
// backward reads it once more and writes the gradient: three sweeps of the live rows in all.  Rows whose label is PAD - most of
// them with captions of ~8 of 29 positions - are never read, and only zero-filled in the backward.
//
// The sweeps of a row - its head / float4 / tail span, the register-resident and the re-reading forward, the sum of exponentials,
// the meets of the four waves, the writer of a gradient row - are vocab_row.h's, shared with reward.hip; here are the visitor
// (arg-max + sum x), the smoothed row loss and the gradient.  No floating-point atomics: per-row results, then a one-workgroup
// reduce that adds them in a fixed order.
#include "vocab_row.h"

namespace {

#define LST ((hipStream_t)stream)
constexpr int LT = CARE_ROW_THREADS;

// forward of one row per workgroup.  NV4 > 0: the row's float4s live in registers (V <= 1024 NV4); NV4 == 0: the
// re-reading form for any V (the second sweep finds the row in the L2).
template <int NV4>
__global__ __launch_bounds__(LT) void lang_loss_fwd_kernel(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq,
                                                           int V, const int32_t* labels, float eps, float* lse, float* rmax,
                                                           float* lsum, float* logp, int32_t* pred, float* row_loss) {
  __shared__ float sm[4];
  __shared__ int si[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int y = labels[r];
  if (y <= 0 || y >= V) {  // PAD, or a label outside [0, V) (counted by the reduce): not read, contributes nothing
    if (tid == 0) { lse[r] = 0.f; rmax[r] = 0.f; lsum[r] = 0.f; logp[r] = 0.f; pred[r] = 0; row_loss[r] = 0.f; }
    return;
  }
  const float* x = logits + (int64_t)(r / rows_per_seq) * seq_stride + (int64_t)(r % rows_per_seq) * ld;
  // arg-max of the row, lowest index on ties, and the sum of its values
  float best = -INFINITY, sx = 0.f;
  int bi = 0x7fffffff;
  auto see = [&](float v, int c) {
    care_argmax_take(best, bi, v, c);
    sx += v;
  };
  care_row<NV4> row;
  row.sweep(x, V, see, [&](const float4& q, int c0) { see(q.x, c0); see(q.y, c0 + 1); see(q.z, c0 + 2); see(q.w, c0 + 3); });
  care_block_argmax4(best, bi, sm, si);
  sx = care_block_sum4(sx, sm);
  const float s = care_block_sum4(row.sum_exp(best), sm);
  if (tid == 0) {
    const float ls = logf(s), L = best + ls;
    const float lp = (x[y] - best) - ls;
    lse[r] = L;
    rmax[r] = best;
    lsum[r] = ls;
    logp[r] = lp;
    pred[r] = bi;
    row_loss[r] = care_smoothed_row_loss(eps, lp, L, sx, V);
  }
}

// sums over rows in a fixed order (one workgroup): thread t adds rows t, t + 1024, ..., the waves' partials meet in LDS
__global__ __launch_bounds__(1024) void lang_loss_reduce_kernel(const float* row_loss, const float* logp, const int32_t* pred,
                                                                const int32_t* labels, int V, int rows, float* sums,
                                                                int32_t* counts, double* acc) {
  __shared__ float fa[16], fb[16];
  __shared__ int ih[16], iw[16], ib[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float a = 0.f, b = 0.f;
  int h = 0, w = 0, bad = 0;
  for (int r = tid; r < rows; r += 1024) {
    const int y = labels[r];
    if (y > 0 && y < V) {
      a += row_loss[r];
      b -= logp[r];
      w += 1;
      h += (pred[r] == y) ? 1 : 0;
    } else if (y != 0) {
      bad += 1;
    }
  }
  a = care_wave_sum(a); b = care_wave_sum(b);
  h = care_wave_sum_i(h); w = care_wave_sum_i(w); bad = care_wave_sum_i(bad);
  if (lane == 0) { fa[wave] = a; fb[wave] = b; ih[wave] = h; iw[wave] = w; ib[wave] = bad; }
  __syncthreads();
  if (tid == 0) {
    a = fa[0]; b = fb[0]; h = ih[0]; w = iw[0]; bad = ib[0];
    for (int q = 1; q < 16; ++q) { a += fa[q]; b += fb[q]; h += ih[q]; w += iw[q]; bad += ib[q]; }
    sums[0] = a; sums[1] = b;
    counts[0] = h; counts[1] = w; counts[2] = bad;
    if (acc) { acc[0] += (double)a; acc[1] += (double)b; acc[2] += (double)h; acc[3] += (double)w; acc[4] += (double)bad; }
  }
}

// backward: one workgroup per row of dlogits (sequence s, position p < seq_rows); live rows one read + one write, the
// others (PAD, bad label, p >= rows_per_seq) a zero fill (vocab_row.h: care_row_zero, care_row_map).
__global__ __launch_bounds__(LT) void lang_loss_bwd_kernel(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq,
                                                           int V, const int32_t* labels, const float* rmax, const float* lsum,
                                                           float eps, const float* g, float* dlogits, int64_t ldd,
                                                           int64_t dseq_stride, int seq_rows) {
  const int s = blockIdx.x / seq_rows, p = blockIdx.x % seq_rows;
  float* d = dlogits + (int64_t)s * dseq_stride + (int64_t)p * ldd;
  int y = 0, r = 0;
  if (p < rows_per_seq) { r = s * rows_per_seq + p; y = labels[r]; }
  const care_row_span sp = care_row_span_of(d, V);
  if (y <= 0 || y >= V) {
    care_row_zero(d, sp);
    return;
  }
  const float* x = logits + (int64_t)s * seq_stride + (int64_t)p * ld;
  // softmax as exp((x - max) - log sum exp(x - max)): x - max is exact for the columns that carry the probability, where
  // x - lse would round at an ulp of |lse| (a row of logits around 5e3: 2e-4 of every probability)
  const float m = rmax[r], ls = lsum[r], gg = *g, sub = eps / (float)V, hot = 1.f - eps;
  care_row_map(x, d, sp, [=](float v, int c) { return gg * ((expf((v - m) - ls) - sub) - (c == y ? hot : 0.f)); });
}

// ------------------------------------------------------------------ concept BCE: one wave per clip
__global__ __launch_bounds__(LT) void noisy_or_bce_fwd_kernel(const float* preds, int64_t ldp, const float* labels, int64_t ldl,
                                                              float* row_loss, float* denom, int B, int K) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* pr = preds + (int64_t)b * ldp;
  const float* yr = labels + (int64_t)b * ldl;
  float s = 0.f, npos = 0.f;
  for (int c = lane; c < K; c += 64) {
    const float p = fminf(fmaxf(pr[c], 0.01f), 0.99f), y = yr[c];
    s += y * logf(p) + (1.f - y) * logf(1.f - p);
    npos += y;
  }
  s = care_wave_sum(s);
  npos = care_wave_sum(npos);
  if (lane == 0) {
    const float den = fmaxf(1.f, npos);
    denom[b] = den;
    row_loss[b] = -s / den;
  }
}

__global__ __launch_bounds__(LT) void noisy_or_bce_bwd_kernel(const float* preds, int64_t ldp, const float* labels, int64_t ldl,
                                                              const float* denom, const float* g, float* dpreds, int64_t ldd,
                                                              int B, int K) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* pr = preds + (int64_t)b * ldp;
  const float* yr = labels + (int64_t)b * ldl;
  float* dr = dpreds + (int64_t)b * ldd;
  const float k = -(*g) / denom[b];
  for (int c = lane; c < K; c += 64) {
    const float p = pr[c], y = yr[c];
    dr[c] = (p >= 0.01f && p <= 0.99f) ? k * (y / p - (1.f - y) / (1.f - p)) : 0.f;  // torch.clamp passes the gradient inside [min, max] only
  }
}

// sum of n floats in a fixed order (one workgroup of 256)
__global__ __launch_bounds__(LT) void sum_reduce_kernel(const float* x, int n, float* sums, double* acc) {
  __shared__ float sm[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += LT) a += x[i];
  a = care_block_sum4(a, sm);
  if (threadIdx.x == 0) {
    sums[0] = a;
    if (acc) acc[0] += (double)a;
  }
}

}  // namespace

extern "C" int care_lang_loss_fwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V,
                                  const int32_t* labels, float eps, float* lse, float* rmax, float* lsum, float* logp,
                                  int32_t* pred, float* row_loss, float* sums, int32_t* counts, double* acc, int rows,
                                  void* stream) {
  const int bad = care_row_check_fwd(logits && labels && lse && rmax && lsum && logp && pred && row_loss && sums && counts, logits, ld,
                                     seq_stride, rows_per_seq, V, rows, eps >= 0.f && eps <= 1.f,
                                     !(acc && ((uintptr_t)acc & 7u)));
  if (bad) return bad;
#define FWD_LAUNCH(N) hipLaunchKernelGGL(lang_loss_fwd_kernel<N>, dim3(rows), dim3(LT), 0, LST, logits, ld, seq_stride, rows_per_seq, V, labels, eps, lse, rmax, lsum, logp, pred, row_loss)
  if (V <= 4096) FWD_LAUNCH(4);
  else if (V <= 8192) FWD_LAUNCH(8);
  else if (V <= 12288) FWD_LAUNCH(12);
  else if (V <= 16384) FWD_LAUNCH(16);
  else FWD_LAUNCH(0);
#undef FWD_LAUNCH
  hipLaunchKernelGGL(lang_loss_reduce_kernel, dim3(1), dim3(1024), 0, LST, row_loss, logp, pred, labels, V, rows, sums, counts, acc);
  return care_launch_status();
}

extern "C" int care_lang_loss_reduce(const float* row_loss, const float* logp, const int32_t* pred, const int32_t* labels, int V,
                                     int rows, float* sums, int32_t* counts, double* acc, void* stream) {
  if (!row_loss || !logp || !pred || !labels || !sums || !counts || rows <= 0 || V <= 0) return CARE_EINVAL;
  if (acc && ((uintptr_t)acc & 7u)) return CARE_EALIGN;
  hipLaunchKernelGGL(lang_loss_reduce_kernel, dim3(1), dim3(1024), 0, LST, row_loss, logp, pred, labels, V, rows, sums, counts, acc);
  return care_launch_status();
}

extern "C" int care_lang_loss_bwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V,
                                  const int32_t* labels, const float* rmax, const float* lsum, float eps, const float* g,
                                  float* dlogits, int64_t ldd, int64_t dseq_stride, int seq_rows, int rows, void* stream) {
  unsigned grid = 0;
  const int bad = care_row_check_bwd(logits && labels && rmax && lsum && g && dlogits, logits, ld, seq_stride, rows_per_seq, V, dlogits,
                                     ldd, dseq_stride, seq_rows, rows, eps >= 0.f && eps <= 1.f, true, &grid);
  if (bad) return bad;
  hipLaunchKernelGGL(lang_loss_bwd_kernel, dim3(grid), dim3(LT), 0, LST, logits, ld, seq_stride, rows_per_seq, V, labels, rmax,
                     lsum, eps, g, dlogits, ldd, dseq_stride, seq_rows);
  return care_launch_status();
}

extern "C" int care_noisy_or_bce_fwd(const float* preds, int64_t ldp, const float* labels, int64_t ldl, float* row_loss,
                                     float* denom, float* sums, double* acc, int B, int K, void* stream) {
  if (!preds || !labels || !row_loss || !denom || !sums || B <= 0 || K <= 0) return CARE_EINVAL;
  if (ldp < K || ldl < K) return CARE_ESHAPE;
  if (acc && ((uintptr_t)acc & 7u)) return CARE_EALIGN;
  hipLaunchKernelGGL(noisy_or_bce_fwd_kernel, dim3((B + 3) / 4), dim3(LT), 0, LST, preds, ldp, labels, ldl, row_loss, denom, B, K);
  hipLaunchKernelGGL(sum_reduce_kernel, dim3(1), dim3(LT), 0, LST, row_loss, B, sums, acc);
  return care_launch_status();
}

extern "C" int care_noisy_or_bce_bwd(const float* preds, int64_t ldp, const float* labels, int64_t ldl, const float* denom,
                                     const float* g, float* dpreds, int64_t ldd, int B, int K, void* stream) {
  if (!preds || !labels || !denom || !g || !dpreds || B <= 0 || K <= 0) return CARE_EINVAL;
  if (ldp < K || ldl < K || ldd < K) return CARE_ESHAPE;
  hipLaunchKernelGGL(noisy_or_bce_bwd_kernel, dim3((B + 3) / 4), dim3(LT), 0, LST, preds, ldp, labels, ldl, denom, g, dpreds, ldd, B, K);
  return care_launch_status();
}
