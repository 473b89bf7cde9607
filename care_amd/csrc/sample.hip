// sample.hip - sampled decoding (include/care_hip.h, care_sample_logits): one token per row drawn from the row's logits under
// temperature, top-k and nucleus (top-p) filtering, handed on through the parts = 1 form of the greedy update's contract
// (pmax = x[tok], pidx = tok, psum = sum exp(x - x[tok])).  fp32 in both library variants.
//
// One workgroup per row, the row in registers: thread `tid` of `nt` owns the columns tid + nt c, c = 0 .. 15 (nt = V / 16
// rounded up to whole waves, at most 1024: V <= 16384 lives in registers; columns beyond that are re-read from memory in
// every pass).  Per column the thread keeps the ordered bit pattern of s = x * inv_temperature and exp(s - max s).
//
// The filters are selections, not sorts.  Both keep a prefix of the order (s descending, index ascending), so the kept set
// is always { key > T } + { key == T and index <= I }:
//   top-k   T = the k-th largest key, built two bits a round from the top - 16 rounds of "how many keys are >= each of three
//           candidates" - and I = the index of the last tie at T that still fits, found the same way over the index bits
//           (only when ties at T have to be cut);
//   top-p   T = the largest key with mass { kept, key >= T } >= top_p Z - 16 rounds of three masked sums in place of the
//           counts - and of the n ties at T the first r with mass { key > T } + j e(T) < top_p Z, j = 0 .. r - 1.
// A round is one pass over the registers and one workgroup reduction with one barrier: within a wave counts and fp32 sums
// come from a DPP scan in a fixed order, the waves meet through LDS and are added in wave order - no atomics, so the same
// inputs give the same bits, and nothing depends on the number of rows.  The masked sums are monotone in the threshold (a
// sum of fixed shape over non-negative terms, the excluded ones replaced by 0), which the bit-by-bit search needs.
// *Measured* (DESIGN.md 9.5): a round costs 0.9 - 1.0 us at V = 10547 (11 waves) - barrier and hand-over, not arithmetic.
//
// The draw is Gumbel-max over the kept set with a counter-based uniform per (seed, row key, step, column): stateless.
#include "care_common.h"

// s = x * inv_temperature is a value of its own (its bit pattern is the selection key): no fused multiply-add with the
// Gumbel term or the maximum
#pragma clang fp contract(off)

namespace {

#define SST ((hipStream_t)stream)
constexpr int SMP_NPT = 16;                      // columns a thread keeps in registers
constexpr int SMP_MAXW = 16;                     // waves of a workgroup
constexpr unsigned SMP_KEY_NEG_INF = 0x007FFFFFu;   // smp_ord(-inf): every finite s orders above it; 0 marks "no column"

// fp32 -> a uint32 that orders like the float (the order csrc/retrieval.hip uses)
__device__ __forceinline__ unsigned smp_ord(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_unord(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct SampleParams {   // the 24-byte device block of care_sample_logits
  unsigned long long seed;
  float inv_temperature, top_p;
  int32_t top_k, reserved;
};

struct SampleArgs {
  const float* logits; int64_t ld; int V;
  const int32_t* row_key; int t;
  const SampleParams* params;
  float* pmax; int32_t* pidx; float* psum; float* logq; int32_t* nkept;
};

// Wave-wide fp32 sum through the DPP data path, in one fixed order: an inclusive scan along each row of 16 lanes (row_shr
// 1, 2, 4, 8; lanes without a source add 0), then row_bcast15 / row_bcast31 carry the row totals to lane 63, which is
// broadcast.  ~8 VALU operations where six xor-shuffles are six dependent trips through the LDS crossbar (care_common.h,
// care_wave_max_dpp).  All 64 lanes must be active.
__device__ __forceinline__ float smp_wave_sum(float v) {
#define SMP_DPP_ADD(CTRL, ROWMASK) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xF, true))
  SMP_DPP_ADD(0x111, 0xF);  // row_shr:1
  SMP_DPP_ADD(0x112, 0xF);  // row_shr:2
  SMP_DPP_ADD(0x114, 0xF);  // row_shr:4
  SMP_DPP_ADD(0x118, 0xF);  // row_shr:8 -> lane 15 of every row holds the row's sum
  SMP_DPP_ADD(0x142, 0xA);  // row_bcast15 into rows 1 and 3
  SMP_DPP_ADD(0x143, 0xC);  // row_bcast31 into rows 2 and 3 -> lane 63 holds the wave's sum
#undef SMP_DPP_ADD
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ unsigned smp_wave_sum(unsigned v) {   // the same scan on integers
#define SMP_DPP_ADD(CTRL, ROWMASK) v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xF, true)
  SMP_DPP_ADD(0x111, 0xF);
  SMP_DPP_ADD(0x112, 0xF);
  SMP_DPP_ADD(0x114, 0xF);
  SMP_DPP_ADD(0x118, 0xF);
  SMP_DPP_ADD(0x142, 0xA);
  SMP_DPP_ADD(0x143, 0xC);
#undef SMP_DPP_ADD
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ __launch_bounds__(1024) void sample_logits_kernel(const SampleArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned red[2][3][SMP_MAXW];
  __shared__ float bestv[SMP_MAXW];
  __shared__ int besti[SMP_MAXW];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nt >> 6;
  const int row = blockIdx.x, V = p.V;
  const float* x = p.logits + (int64_t)row * p.ld;
  const unsigned long long seed = p.params->seed;
  const float inv_t = p.params->inv_temperature, top_p = p.params->top_p;
  const int top_k = p.params->top_k;

  // ---- workgroup reductions of up to three values at once: every thread calls them, the waves' sums (smp_wave_sum) meet
  // in LDS, every thread gets the 16 per-wave values back (waves the launch does not have: 0) and combines them in wave
  // order.  Round r writes red[r & 1]; the barrier of round r + 1 lies between a wave's reads of round r and
  // anybody's writes of round r + 2.
  for (int i = tid; i < 2 * 3 * SMP_MAXW; i += nt) (&red[0][0][0])[i] = 0u;
  __syncthreads();
  int round = 0;
  auto exchange = [&](const unsigned* mine, int n, unsigned (*all)[SMP_MAXW]) {
    const int b = round & 1;
    ++round;
    if (lane == 0)
      for (int j = 0; j < n; ++j) red[b][j][w] = mine[j];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const u32x4* r4 = reinterpret_cast<const u32x4*>(red[b][j]);
#pragma unroll
      for (int q = 0; q < SMP_MAXW / 4; ++q) {
        const u32x4 v = r4[q];
        all[j][4 * q] = v[0]; all[j][4 * q + 1] = v[1]; all[j][4 * q + 2] = v[2]; all[j][4 * q + 3] = v[3];
      }
    }
  };
  auto block_sum_u = [&](unsigned (&c)[3], int n) {
    unsigned all[3][SMP_MAXW];
    for (int j = 0; j < n; ++j) c[j] = smp_wave_sum(c[j]);
    exchange(c, n, all);
    for (int j = 0; j < n; ++j) {
      unsigned s = 0;
#pragma unroll
      for (int k = 0; k < SMP_MAXW; ++k) s += all[j][k];
      c[j] = s;
    }
  };
  auto block_sum_f = [&](float (&a)[3], int n) {
    unsigned mine[3], all[3][SMP_MAXW];
    for (int j = 0; j < n; ++j) mine[j] = __builtin_bit_cast(unsigned, smp_wave_sum(a[j]));
    exchange(mine, n, all);
    for (int j = 0; j < n; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < SMP_MAXW; ++k) s += __builtin_bit_cast(float, all[j][k]);
      a[j] = s;
    }
  };

  // ---- the row: key of s (0: no such column), later exp(s - m)
  auto key_of = [&](float xv) -> unsigned { return smp_ord(xv * inv_t + 0.0f); };   // (+ 0: -0 orders as +0)
  float ex[SMP_NPT];
  unsigned key[SMP_NPT];
  unsigned kmax = 0;
#pragma unroll
  for (int c = 0; c < SMP_NPT; ++c) {
    const int i = tid + nt * c;
    key[c] = i < V ? key_of(x[i]) : 0u;
    kmax = max(kmax, key[c]);
  }
  const int tail0 = SMP_NPT * nt;   // columns from here on (only with nt = 1024 and V > 16384) are re-read in every pass
  for (int base = tail0; base < V; base += nt) kmax = max(kmax, base + tid < V ? key_of(x[base + tid]) : 0u);
  {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor(kmax, o, 64));
    unsigned all[1][SMP_MAXW];
    exchange(&kmax, 1, all);
#pragma unroll
    for (int k = 0; k < SMP_MAXW; ++k) kmax = max(kmax, all[0][k]);
  }
  if (kmax <= SMP_KEY_NEG_INF) {   // no finite entry: nothing to draw from
    if (tid == 0) {
      p.pidx[row] = 0; p.pmax[row] = x[0]; p.psum[row] = 1.f;
      if (p.logq) p.logq[row] = 0.f;
      if (p.nkept) p.nkept[row] = 0;
    }
    return;
  }
  const float m = smp_unord(kmax);
  auto exp_of = [&](unsigned k) -> float { return k > SMP_KEY_NEG_INF ? expf(smp_unord(k) - m) : 0.f; };
#pragma unroll
  for (int c = 0; c < SMP_NPT; ++c) ex[c] = exp_of(key[c]);

  // counts / masses of up to three predicates in ONE pass over the row and one workgroup reduction: pred(j, key, index)
  auto count_if = [&](auto pred, int n, unsigned (&out)[3]) {
    out[0] = out[1] = out[2] = 0;
#pragma unroll
    for (int c = 0; c < SMP_NPT; ++c)
      for (int j = 0; j < n; ++j) out[j] += pred(j, key[c], tid + nt * c) ? 1u : 0u;
    for (int base = tail0; base < V; base += nt) {
      const int i = base + tid;
      const unsigned k = i < V ? key_of(x[i]) : 0u;
      for (int j = 0; j < n; ++j) out[j] += pred(j, k, i) ? 1u : 0u;
    }
    block_sum_u(out, n);
  };
  auto count1 = [&](auto pred) -> unsigned {
    unsigned out[3];
    count_if([&](int, unsigned k, int i) { return pred(k, i); }, 1, out);
    return out[0];
  };
  auto mass_if = [&](auto pred, int n, float (&out)[3]) {
    out[0] = out[1] = out[2] = 0.f;
#pragma unroll
    for (int c = 0; c < SMP_NPT; ++c)
      for (int j = 0; j < n; ++j) out[j] += pred(j, key[c], tid + nt * c) ? ex[c] : 0.f;
    for (int base = tail0; base < V; base += nt) {
      const int i = base + tid;
      const unsigned k = i < V ? key_of(x[i]) : 0u;
      const float e = exp_of(k);
      for (int j = 0; j < n; ++j) out[j] += pred(j, k, i) ? e : 0.f;
    }
    block_sum_f(out, n);
  };
  auto mass1 = [&](auto pred) -> float {
    float out[3];
    mass_if([&](int, unsigned k, int i) { return pred(k, i); }, 1, out);
    return out[0];
  };

  // the kept set: key > Tx, or key == Te and index <= Ie.  At first every finite entry.  (No column has key 0 but the
  // padding slots, whose index is >= V > Ie.)
  unsigned Tx = SMP_KEY_NEG_INF, Te = 0u;
  int Ie = -1;
  auto kept = [&](unsigned k, int i) -> bool { return k > Tx || (k == Te && i <= Ie); };
  // the index of the r-th (1-based) lowest column among those with key T and index <= lim: the largest I with fewer than
  // r of them below I
  const int idx_bits = V > 1 ? 32 - __builtin_clz((unsigned)(V - 1)) : 0;
  auto kth_index = [&](unsigned T, unsigned r, int lim) -> int {
    unsigned I = 0;
    for (int bit = idx_bits - 1; bit >= 0; --bit) {
      const unsigned cand = I | (1u << bit);
      if (count1([&](unsigned k, int i) { return k == T && i <= lim && (unsigned)i < cand; }) < r) I = cand;
    }
    return (int)I;
  };

  // ---- top-k
  const unsigned nfin = count1([&](unsigned k, int) { return k > SMP_KEY_NEG_INF; });
  if (top_k > 0 && (unsigned)top_k < nfin) {
    const unsigned K = (unsigned)top_k;
    unsigned T = 0;   // the largest T with K or more keys >= T, two bits a round
    for (int lo = 30; lo >= 0; lo -= 2) {
      unsigned n3[3];
      count_if([&](int j, unsigned k, int) { return k >= (T | ((unsigned)(j + 1) << lo)); }, 3, n3);
      T |= (n3[2] >= K ? 3u : n3[1] >= K ? 2u : n3[0] >= K ? 1u : 0u) << lo;
    }
    unsigned n2[3];
    count_if([&](int j, unsigned k, int) { return j == 0 ? k > T : k == T; }, 2, n2);
    const unsigned need = K - n2[0];   // (n2[0] < K: keys above T)
    const int I = need < n2[1] ? kth_index(T, need, 0x7FFFFFFF) : 0x7FFFFFFF;
    Tx = T; Te = T; Ie = I;
  }

  // ---- top-p over what top-k left
  if (top_p < 1.f) {
    const float Z = mass1(kept);
    const float P = fmaxf(top_p, 1e-30f) * Z;   // (> 0 and <= Z)
    unsigned T = 0;   // the largest T with mass { kept, key >= T } >= P, two bits a round
    for (int lo = 30; lo >= 0; lo -= 2) {
      float m3[3];
      mass_if([&](int j, unsigned k, int i) { return k >= (T | ((unsigned)(j + 1) << lo)) && kept(k, i); }, 3, m3);
      T |= (m3[2] >= P ? 3u : m3[1] >= P ? 2u : m3[0] >= P ? 1u : 0u) << lo;
    }
    // T is a kept key: mass { key > T } < P <= mass { key >= T }
    const float mgt = mass1([&](unsigned k, int i) { return k > T && kept(k, i); });
    const unsigned neq = count1([&](unsigned k, int i) { return k == T && kept(k, i); });
    const float ev = exp_of(T);
    unsigned r = neq;
    if (neq > 1 && ev > 0.f) {   // tie j (0-based, by index) stays while mgt + j ev < P
      const float est = fminf(fmaxf(ceilf((P - mgt) / ev), 1.f), (float)neq);
      r = (unsigned)est;
      while (r > 1 && !(mgt + (float)(r - 1) * ev < P)) --r;
      while (r < neq && (mgt + (float)r * ev < P)) ++r;
    }
    const int lim = Te == T ? Ie : 0x7FFFFFFF;
    const int I = r < neq ? kth_index(T, r, lim) : lim;
    Tx = T; Te = T; Ie = I;
  }
  const float Zk = mass1(kept);
  const unsigned nk = count1(kept);

  // ---- Gumbel-max over the kept set; ties to the lower index
  const unsigned rk = p.row_key ? (unsigned)p.row_key[row] : (unsigned)row;
  const unsigned long long rs = care_mix64(seed,((unsigned long long)rk << 16) | (unsigned long long)(unsigned)p.t);
  auto perturbed = [&](unsigned k, int i) -> float {
    const unsigned kk = (unsigned)(care_mix64(rs, (unsigned long long)i) >> 41);  // the top 23 bits
    const float u = (float)(2u * kk + 1u) * (1.0f / 16777216.0f);                   // exact, in (0, 1)
    return smp_unord(k) + (-logf(-logf(u)));
  };
  float bv = -INFINITY;
  int bi = 0x7FFFFFFF;
#pragma unroll
  for (int c = 0; c < SMP_NPT; ++c) {
    const int i = tid + nt * c;
    if (kept(key[c], i)) {
      const float v = perturbed(key[c], i);
      if (v > bv || bi == 0x7FFFFFFF) { bv = v; bi = i; }
    }
  }
  for (int i = tail0 + tid; i < V; i += nt) {
    const unsigned k = key_of(x[i]);
    if (kept(k, i)) {
      const float v = perturbed(k, i);
      if (v > bv || bi == 0x7FFFFFFF) { bv = v; bi = i; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  if (lane == 0) { bestv[w] = bv; besti[w] = bi; }
  __syncthreads();
  bv = bestv[0]; bi = besti[0];
  for (int k = 1; k < nw; ++k) {
    const float ov = bestv[k];
    const int oi = besti[k];
    if (oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  const int tok = bi == 0x7FFFFFFF ? 0 : bi;   // (a kept set is never empty)

  // ---- the model's own statistics of the chosen token, over all V columns at temperature 1
  const float xt = x[tok];
  float a3[3] = {0.f, 0.f, 0.f};
  for (int base = 0; base < V; base += nt) a3[0] += base + tid < V ? expf(x[base + tid] - xt) : 0.f;   // (the logits once more: s does not give x back)
  block_sum_f(a3, 1);
  if (tid == 0) {
    p.pmax[row] = xt; p.pidx[row] = tok; p.psum[row] = a3[0];
    if (p.logq) p.logq[row] = (smp_unord(key_of(xt)) - m) - logf(Zk);
    if (p.nkept) p.nkept[row] = (int)nk;
  }
}

__global__ __launch_bounds__(256) void sample_accum_kernel(const float* __restrict__ logq, const int32_t* __restrict__ finished,
                                                           float* __restrict__ score_q, int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < rows && finished[r] == 0) score_q[r] += logq[r];
}

}  // namespace

extern "C" int care_sample_logits(const float* logits, int64_t ld, int V, int rows, const int32_t* row_key, int t,
                                  const void* params, float* pmax, int32_t* pidx, float* psum, float* logq, int32_t* nkept,
                                  void* stream) {
  if (rows < 0 || V < 1 || ld < V || t < 1 || !logits || !params || !pmax || !pidx || !psum) return CARE_EINVAL;
  if (!care_aligned16(params)) return CARE_EALIGN;
  if (rows == 0) return 0;
  SampleArgs p;
  p.logits = logits; p.ld = ld; p.V = V; p.row_key = row_key; p.t = t;
  p.params = static_cast<const SampleParams*>(params);
  p.pmax = pmax; p.pidx = pidx; p.psum = psum; p.logq = logq; p.nkept = nkept;
  // V / 16 threads in whole waves: by V alone, so a row meets the same reduction tree in every batch
  int nt = ((V + SMP_NPT - 1) / SMP_NPT + 63) / 64 * 64;
  nt = nt > 64 * SMP_MAXW ? 64 * SMP_MAXW : nt;
  hipLaunchKernelGGL(sample_logits_kernel, dim3((unsigned)rows), dim3((unsigned)nt), 0, SST, p);
  return care_launch_status();
}

extern "C" int care_sample_accum(const float* logq, const int32_t* finished, float* score_q, int rows, void* stream) {
  if (rows < 0 || !logq || !finished || !score_q) return CARE_EINVAL;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(sample_accum_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, SST, logq, finished, score_q, rows);
  return care_launch_status();
}
