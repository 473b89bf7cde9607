// head_reward.hip - the small kernels around the training head fused with the SELF-CRITICAL loss (include/care_hip.h, "The
// training head fused with the self-critical loss"; care_amd/reward.py, _HeadRewardLoss): the vocabulary projection of
// models/Head.py:26-32 and the advantage-weighted log-likelihood of care_reward_loss_fwd over the LIVE label positions only,
// the logits never in memory.  The products are head_loss.hip's: care_head_live_rows, care_gemm_tile_split3_head_stats and
// care_gemm_tile_split3_head_grad (eps = 0) as they are.  The weight of a row - its caption's advantage - is linear in the
// gradient, so it never enters the [R, V] side: it multiplies the d-wide rows on either side of the two gradient products.
//
//   care_head_reward_finish  the parts of a row -> max, log sum exp(x - max), logp and the row's weight (one wave per row);
//   care_head_reward_reduce  sum w logp, the loss, each caption's sum of logp (one workgroup, double, one order);
//   care_head_reward_gscale  g / n_live as a device float and |g / n_live| as the |max| slot of the gradient's pieces;
//   care_rows_scale          dst[i, :] = w[i] src[i, :]  (w (.) h_live in front of dW's pieces, w (.) dh_live behind dh's product).
// No floating-point atomics anywhere: every sum has one order.  fp32 / double in both library variants.
#include "caption_core.h"

namespace {

#define RST ((hipStream_t)stream)

// One wave per live row, head_loss.hip's merge without the arg-max: lane l takes parts l, l + 64, ... in ascending order, the
// lanes meet in xor steps - care_head_loss_finish's rmax, lsum and logp bit for bit.
__global__ __launch_bounds__(256) void head_reward_finish_kernel(const float* pmax, const float* psum, const float* plab, int parts,
                                                                 const int32_t* idx_l, const float* adv, int t, int R, float* rmax_c,
                                                                 float* lsum_c, float* logp_c, float* w_c) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= R) return;
  const int64_t o = (int64_t)i * parts;
  float best = -INFINITY;
  for (int k = lane; k < parts; k += 64) best = fmaxf(best, pmax[o + k]);
  best = care_wave_max(best);
  float s = 0.f, lv = -INFINITY;
  for (int k = lane; k < parts; k += 64) {
    s += psum[o + k] * expf(pmax[o + k] - best);
    lv = fmaxf(lv, plab[o + k]);
  }
  s = care_wave_sum(s);
  lv = care_wave_max(lv);
  if (lane == 0) {
    const float ls = logf(s);
    rmax_c[i] = best;
    lsum_c[i] = ls;
    logp_c[i] = (lv - best) - ls;
    w_c[i] = adv[idx_l[i] / t];
  }
}

// One workgroup.  The weighted sum: thread q adds the live rows q, q + 1024, ... in double, a scan in lane order, the waves in
// wave order (care_reward_loss_fwd's reduction over the compact rows).  A row whose weight is exactly 0 adds nothing.  The
// captions: idx_l ascends, so a caption's live rows are one run of the compact arrays, found by binary search and added in
// position order.
__global__ __launch_bounds__(1024) void head_reward_reduce_kernel(const float* logp_c, const float* w_c, const int32_t* idx_l, int R,
                                                                  int t, int n_seq, double* totals, float* loss, float* seq_logp,
                                                                  double* acc) {
  __shared__ double sa[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a = 0.0;
  for (int i = tid; i < R; i += 1024) {
    const float w = w_c[i];
    if (w != 0.f) a += (double)w * (double)logp_c[i];
  }
  a = care_wave_scan_total(a);
  if (lane == 0) sa[wave] = a;
  __syncthreads();
  if (tid == 0) {
    a = sa[0];
    for (int q = 1; q < 16; ++q) a += sa[q];
    const float l = R > 0 ? (float)(-(a / (double)R)) : 0.f;
    totals[0] = a;
    totals[1] = (double)R;
    *loss = l;
    if (acc) { acc[0] += (double)l; acc[1] += (double)R; }
  }
  if (seq_logp) {
    for (int s = tid; s < n_seq; s += 1024) {
      const int64_t first = (int64_t)s * t, end = first + t;
      int lo = 0, hi = R;
      while (lo < hi) {   // the first live row at or behind the caption's first position
        const int mid = lo + ((hi - lo) >> 1);
        if (idx_l[mid] < first) lo = mid + 1;
        else hi = mid;
      }
      double sum = 0.0;
      for (int i = lo; i < R && idx_l[i] < end; ++i) sum += (double)logp_c[i];
      seq_logp[s] = (float)sum;
    }
  }
}

__global__ void head_reward_gscale_kernel(const float* g, const double* totals, float* gs, unsigned* slot) {
  const double n = totals[1];
  const float v = n > 0.0 ? (float)((double)(*g) / n) : 0.f;
  *gs = v;
  *slot = __builtin_bit_cast(unsigned, v) & 0x7fffffffu;
}

// One thread per element group: T = float4 when columns, strides and pointers allow 16-byte accesses, float otherwise.
template <class T>
__global__ __launch_bounds__(256) void rows_scale_kernel(const float* src, int64_t lds, const float* w, float* dst, int64_t ldd,
                                                         int64_t total, int per_row) {
  constexpr int E = sizeof(T) / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t r = i / per_row;
  const int c = (int)(i - r * per_row) * E;
  const float f = w[r];
  if constexpr (E == 4) {
    float4 v = *reinterpret_cast<const float4*>(src + r * lds + c);
    v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    *reinterpret_cast<float4*>(dst + r * ldd + c) = v;
  } else {
    dst[r * ldd + c] = f * src[r * lds + c];
  }
}

}  // namespace

extern "C" int care_head_reward_finish(const float* pmax, const float* psum, const float* plab, int parts, const int32_t* idx_l,
                                       const float* adv, int t, int V, int R, float* rmax_c, float* lsum_c, float* logp_c,
                                       float* w_c, void* stream) {
  if (!pmax || !psum || !plab || !idx_l || !adv || !rmax_c || !lsum_c || !logp_c || !w_c || R < 0 || V <= 0 || t <= 0)
    return CARE_EINVAL;
  if (parts != (V + 63) / 64) return CARE_ESHAPE;
  if (R == 0) return 0;
  hipLaunchKernelGGL(head_reward_finish_kernel, dim3((R + 3) / 4), dim3(256), 0, RST, pmax, psum, plab, parts, idx_l, adv, t, R, rmax_c,
                     lsum_c, logp_c, w_c);
  return care_launch_status();
}

extern "C" int care_head_reward_reduce(const float* logp_c, const float* w_c, const int32_t* idx_l, int R, int t, int n_seq,
                                       double* totals, float* loss, float* seq_logp, double* acc, void* stream) {
  if (!logp_c || !w_c || !idx_l || !totals || !loss || R < 0 || t <= 0 || n_seq <= 0) return CARE_EINVAL;
  if ((int64_t)n_seq * t > 0x7fffffff || R > (int64_t)n_seq * t) return CARE_ESHAPE;
  if (!care_aligned8(totals) || !care_aligned8(acc)) return CARE_EALIGN;
  hipLaunchKernelGGL(head_reward_reduce_kernel, dim3(1), dim3(1024), 0, RST, logp_c, w_c, idx_l, R, t, n_seq, totals, loss, seq_logp,
                     acc);
  return care_launch_status();
}

extern "C" int care_head_reward_gscale(const float* g, const double* totals, float* gs, void* slot, void* stream) {
  if (!g || !totals || !gs || !slot) return CARE_EINVAL;
  if (!care_aligned8(totals)) return CARE_EALIGN;
  hipLaunchKernelGGL(head_reward_gscale_kernel, dim3(1), dim3(1), 0, RST, g, totals, gs, reinterpret_cast<unsigned*>(slot));
  return care_launch_status();
}

extern "C" int care_rows_scale(const float* src, int64_t ld_src, const float* w, float* dst, int64_t ld_dst, int rows, int cols,
                               void* stream) {
  if (!src || !w || !dst || rows < 0 || cols < 0) return CARE_EINVAL;
  if (ld_src < cols || ld_dst < cols) return CARE_ESHAPE;
  if (rows == 0 || cols == 0) return 0;
  const bool v16 = !(cols % 4) && !(ld_src % 4) && !(ld_dst % 4) && care_aligned16(src) && care_aligned16(dst);
  const int per_row = v16 ? cols / 4 : cols;
  const int64_t total = (int64_t)rows * per_row, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return CARE_ESHAPE;
  if (v16) hipLaunchKernelGGL(rows_scale_kernel<float4>, dim3((unsigned)blocks), dim3(256), 0, RST, src, ld_src, w, dst, ld_dst, total, per_row);
  else hipLaunchKernelGGL(rows_scale_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, RST, src, ld_src, w, dst, ld_dst, total, per_row);
  return care_launch_status();
}
