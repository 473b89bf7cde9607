// head_loss.hip - the small kernels around the training head fused with the language loss (include/care_hip.h, "The training
// head fused with the language loss"; care_amd/criterion.py, _HeadLoss): the vocabulary projection of models/Head.py:26-32 and
// the label-smoothed NLL of misc/Crit/crit_lang.py:49-71 over the LIVE label positions only, the logits never in memory.
//
//   care_head_live_rows   labels -> the ordered index of the live positions, their count, the count of bad labels;
//   (csrc/gemm_tile.hip)  care_gemm_tile_split3_head_stats: per (row, 64-column part) max / first arg-max / sum exp / label
//                         logit / sum x of the split product's accumulators;
//   care_head_loss_finish the parts of a row -> max, log sum exp(x - max), logp, prediction, row loss (one wave per row);
//   (csrc/loss.hip)       care_lang_loss_reduce: the rows added in care_lang_loss_fwd's fixed order;
//   care_head_grad_scale  |g| of the upstream device scalar as the |max| slot of the gradient's pieces (|dl| <= |g|);
//   (csrc/gemm_tile.hip)  care_gemm_tile_split3_head_grad: the product again, dl written as scaled fp16 pieces [R, 2 ks];
//   care_pieces_transpose those pieces -> the slab-major pieces of dl^T (the A operand of dW = dl^T h), fp16 to fp16.
// No floating-point atomics anywhere: every sum has one order.
#include "care_common.h"

namespace {

#define HST ((hipStream_t)stream)

// One workgroup: thread t owns the positions t per .. t per + per - 1, counts its live ones, an exclusive scan over the
// threads gives its first output slot - ascending order by construction.
__global__ __launch_bounds__(1024) void head_live_rows_kernel(const int32_t* labels, int rows, int t, int seq_rows, int V,
                                                              int32_t* idx_h, int32_t* idx_l, int32_t* lab_c, int32_t* counts) {
  __shared__ int wl[16], wb[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (rows + 1023) / 1024;
  const int r0 = min(tid * per, rows), r1 = min(r0 + per, rows);
  int live = 0, bad = 0;
  for (int r = r0; r < r1; ++r) {
    const int y = labels[r];
    live += (y > 0 && y < V) ? 1 : 0;
    bad += (y < 0 || y >= V) ? 1 : 0;
  }
  int inc = live;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  bad = care_wave_sum_i(bad);
  if (lane == 63) wl[wave] = inc;
  if (lane == 0) wb[wave] = bad;
  __syncthreads();
  int at = inc - live;
  for (int w = 0; w < wave; ++w) at += wl[w];
  for (int r = r0; r < r1; ++r) {
    const int y = labels[r];
    if (y > 0 && y < V) {
      idx_h[at] = (r / t) * seq_rows + r % t;
      idx_l[at] = r;
      lab_c[at] = y;
      ++at;
    }
  }
  if (tid == 0) {
    int a = 0, b = 0;
    for (int w = 0; w < 16; ++w) { a += wl[w]; b += wb[w]; }
    counts[0] = a;
    counts[1] = b;
  }
}

// One wave per live row: lane l merges parts l, l + 64, ...; the lanes meet in xor steps (lowest column on equal maxima).
__global__ __launch_bounds__(256) void head_finish_kernel(const float* pmax, const int32_t* pidx, const float* psum, const float* plab,
                                                          const float* psx, int parts, const int32_t* lab_c, const int32_t* idx_l,
                                                          int V, float eps, int R, float* lse, float* rmax, float* lsum, float* logp,
                                                          int32_t* pred, float* row_loss, float* rmax_c, float* lsum_c) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= R) return;
  const int64_t o = (int64_t)i * parts;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int k = lane; k < parts; k += 64) care_argmax_take(best, bi, pmax[o + k], pidx[o + k]);
  care_wave_argmax(best, bi);
  float s = 0.f, sx = 0.f, lv = -INFINITY;
  for (int k = lane; k < parts; k += 64) {
    s += psum[o + k] * expf(pmax[o + k] - best);
    sx += psx[o + k];
    lv = fmaxf(lv, plab[o + k]);
  }
  s = care_wave_sum(s);
  sx = care_wave_sum(sx);
  lv = care_wave_max(lv);
  if (lane == 0) {
    const float ls = logf(s), L = best + ls;
    const float lp = (lv - best) - ls;
    const int r = idx_l[i];
    lse[r] = L;
    rmax[r] = best;
    lsum[r] = ls;
    logp[r] = lp;
    pred[r] = bi;
    row_loss[r] = care_smoothed_row_loss(eps, lp, L, sx, V);
    rmax_c[i] = best;
    lsum_c[i] = ls;
  }
}

__global__ void head_grad_scale_kernel(const float* g, unsigned* slot) { *slot = __builtin_bit_cast(unsigned, *g) & 0x7fffffffu; }

// 64 x 64 tiles of each piece through LDS: reads along v (the source's contiguous dimension), writes along k.
__global__ __launch_bounds__(256) void pieces_transpose_kernel(const _Float16* src, int R, int V, int ks_v, int ks_r, _Float16* out) {
  __shared__ _Float16 tile[64][66];
  const int tiles_v = (V + 63) >> 6;
  const int tv = blockIdx.x % tiles_v, tr = blockIdx.x / tiles_v;
  const int v0 = tv * 64, r0 = tr * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int slab = r0 / ks_r, k0 = r0 - slab * ks_r;  // a 64-row tile lies inside one slab (ks_r % 64 == 0)
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int r = r0 + p * 4 + ty;  // v0 + tx < ks_v: ks_v % 64 == 0 and V <= ks_v
      tile[p * 4 + ty][tx] = r < R ? src[(int64_t)r * 2 * ks_v + (int64_t)q * ks_v + v0 + tx] : (_Float16)0.f;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int vv = p * 4 + ty, v = v0 + vv;
      if (v < V) out[((int64_t)slab * V + v) * 2 * ks_r + (int64_t)q * ks_r + k0 + tx] = tile[tx][vv];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int care_head_live_rows(const int32_t* labels, int n_seq, int t, int seq_rows, int V, int32_t* idx_h, int32_t* idx_l,
                                   int32_t* lab_c, int32_t* counts, void* stream) {
  if (!labels || !idx_h || !idx_l || !lab_c || !counts || n_seq <= 0 || t <= 0 || V <= 0) return CARE_EINVAL;
  if (seq_rows < t || (int64_t)n_seq * seq_rows > 0x7fffffff) return CARE_ESHAPE;
  hipLaunchKernelGGL(head_live_rows_kernel, dim3(1), dim3(1024), 0, HST, labels, n_seq * t, t, seq_rows, V, idx_h, idx_l, lab_c, counts);
  return care_launch_status();
}

extern "C" int care_head_loss_finish(const float* pmax, const int32_t* pidx, const float* psum, const float* plab, const float* psx,
                                     int parts, const int32_t* lab_c, const int32_t* idx_l, int V, float eps, int R, float* lse,
                                     float* rmax, float* lsum, float* logp, int32_t* pred, float* row_loss, float* rmax_c,
                                     float* lsum_c, void* stream) {
  if (!pmax || !pidx || !psum || !plab || !psx || !lab_c || !idx_l || !lse || !rmax || !lsum || !logp || !pred || !row_loss ||
      !rmax_c || !lsum_c || R <= 0 || V <= 0)
    return CARE_EINVAL;
  if (parts != (V + 63) / 64 || !(eps >= 0.f && eps <= 1.f)) return CARE_ESHAPE;
  hipLaunchKernelGGL(head_finish_kernel, dim3((R + 3) / 4), dim3(256), 0, HST, pmax, pidx, psum, plab, psx, parts, lab_c, idx_l, V, eps,
                     R, lse, rmax, lsum, logp, pred, row_loss, rmax_c, lsum_c);
  return care_launch_status();
}

extern "C" int care_head_grad_scale(const float* g, void* slot, void* stream) {
  if (!g || !slot) return CARE_EINVAL;
  hipLaunchKernelGGL(head_grad_scale_kernel, dim3(1), dim3(1), 0, HST, g, reinterpret_cast<unsigned*>(slot));
  return care_launch_status();
}

extern "C" int care_pieces_transpose(const void* src, int R, int V, int ks_v, int slabs, int ks_r, void* out, void* stream) {
  if (!src || !out || R <= 0 || V <= 0 || slabs <= 0 || ks_v <= 0 || ks_r <= 0) return CARE_EINVAL;
  if (ks_v % 64 != 0 || ks_r % 64 != 0 || V > ks_v || (int64_t)slabs * ks_r < R) return CARE_ESHAPE;
  const int64_t blocks = (int64_t)((V + 63) / 64) * (((int64_t)slabs * ks_r) >> 6);
  if (blocks > 0x7fffffff) return CARE_ESHAPE;
  hipLaunchKernelGGL(pieces_transpose_kernel, dim3((unsigned)blocks), dim3(256), 0, HST, reinterpret_cast<const _Float16*>(src), R, V,
                     ks_v, ks_r, reinterpret_cast<_Float16*>(out));
  return care_launch_status();
}
