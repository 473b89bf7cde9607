// concept_metrics.hip - F1@k and average precision of the concept probabilities against multi-hot labels
// (include/care_hip.h, "Concept metrics"): the metric half of NoisyOrMIL._step (misc/Crit/crit_attribute.py:58-89) without a
// sort, and its sums over an epoch in a totals block that stays on the device.  int / fp32 compares / double in both library
// variants; no floating-point atomics; a clip's bits depend on the clip alone (the rules of capmetrics.hip).
//
// Every metric is a function of two integers per positive column j of a clip: rank_j, the number of columns before j, and
// posrank_j, the number of POSITIVE columns before j, in ONE total order: the clamped probability descending, NaN before every
// number, the lower column first among equals.  A clamped probability is a positive float, so its bit pattern orders like the
// value; NaN becomes the largest key: "i before j" is  key_i > key_j || (key_i == key_j && i < j)  on uint32 keys in LDS.
// One workgroup of four waves per clip: the keys and a bitmap of the positives (one ballot a chunk of 64 columns) in LDS, the
// positives compacted in ascending column order (the bitmap's popcounts), dealt to the waves; for one positive the 64 lanes
// sweep the K columns counting both integers (packed into one int), one wave reduction; rank is stored at slot posrank (the
// posranks are a permutation of 0 .. P - 1).  AP = (sum_s (s + 1) / (rank[s] + 1)) / P in double, summed in one fixed order
// (the lane-order scan of csrc/caption_core.h).
#include "caption_core.h"

// (each double operation rounded on its own, in both libraries)
#pragma clang fp contract(off)

namespace {

#define CST ((hipStream_t)stream)
constexpr int QT = 256;                          // threads of a clip's workgroup (4 waves)
constexpr int QW = QT / 64;
constexpr int QK = CARE_CONCEPT_MAX_K;           // columns the LDS form holds
constexpr int QC = QK / 64;                      // chunks of 64 columns
constexpr int QN = CARE_CONCEPT_MAX_TOPK;
constexpr int TT = 1024;                         // threads of the totals workgroup (16 waves)

struct TopK { int k[QN]; };

// clamp(p, 0.01, 0.99) as torch.clamp does it (NaN stays NaN), as a key that orders like the value with NaN on top
__device__ __forceinline__ uint32_t q_key(float p) {
  if (p != p) return 0xFFFFFFFFu;
  const float c = p < 0.01f ? 0.01f : (p > 0.99f ? 0.99f : p);
  return __builtin_bit_cast(uint32_t, c);
}

__global__ __launch_bounds__(QT) void concept_metrics_kernel(const float* preds, int64_t ldp, const float* labels, int64_t ldl,
                                                             int K, TopK topk, int n_topk, double* ap, int32_t* hits,
                                                             int32_t* n_pos) {
  __shared__ uint32_t s_key[QK];
  __shared__ int32_t s_rank[QK];                 // slot posrank -> rank
  __shared__ uint16_t s_list[QK];                // the positive columns, ascending
  __shared__ unsigned long long s_bits[QC];      // bit c of word q: column 64 q + c is positive
  __shared__ int32_t s_base[QC + 1];             // positives before chunk q; [chunks] = P
  __shared__ int32_t s_hits[QW][QN];
  __shared__ double s_sum[QW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunks = (K + 63) >> 6;
  const float* p = preds + (int64_t)b * ldp;
  const float* y = labels + (int64_t)b * ldl;

  for (int q = wave; q < chunks; q += QW) {
    const int c = (q << 6) + lane;
    bool pos = false;
    if (c < K) {
      s_key[c] = q_key(p[c]);
      pos = y[c] != 0.f;
    }
    const unsigned long long m = __ballot(pos);
    if (lane == 0) s_bits[q] = m;
  }
  __syncthreads();
  if (wave == 0) {   // chunks <= 64: an exclusive scan of the chunks' counts over the lanes
    const int n = lane < chunks ? __popcll(s_bits[lane]) : 0;
    int v = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane < chunks) s_base[lane] = v - n;
    if (lane == 63) s_base[chunks] = v;
  }
  __syncthreads();
  const int P = s_base[chunks];
  for (int q = wave; q < chunks; q += QW) {
    const unsigned long long m = s_bits[q];
    if ((m >> lane) & 1ull) s_list[s_base[q] + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)((q << 6) + lane);
  }
  __syncthreads();

  int wh[QN];
#pragma unroll
  for (int t = 0; t < QN; ++t) wh[t] = 0;
  for (int s = wave; s < P; s += QW) {
    const int j = s_list[s];
    const uint32_t kj = s_key[j];
    int cnt = 0;                                 // rank + (posrank << 16): both <= K - 1 < 2^13, 64 lanes' sum < 2^16 each
    for (int q = 0; q < chunks; ++q) {
      const int c = (q << 6) + lane;
      if (c < K) {
        const uint32_t kc = s_key[c];
        const bool before = kc > kj || (kc == kj && c < j);
        const int bit = (int)((s_bits[q] >> lane) & 1ull);
        cnt += before ? 1 + (bit << 16) : 0;
      }
    }
    cnt = care_wave_sum_i(cnt);
    const int rank = cnt & 0xFFFF, posrank = cnt >> 16;
    if (lane == 0) s_rank[posrank] = rank;
#pragma unroll
    for (int t = 0; t < QN; ++t) wh[t] += (t < n_topk && rank < topk.k[t]) ? 1 : 0;
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < QN; ++t) s_hits[wave][t] = wh[t];
  }
  __syncthreads();

  // AP: thread t owns the slots t, t + 256, ..; a scan in lane order; the waves in wave order
  double part = 0.0;
  for (int s = tid; s < P; s += QT) part += (double)(s + 1) / (double)(s_rank[s] + 1);
  part = care_wave_scan_total(part);
  if (lane == 0) s_sum[wave] = part;
  __syncthreads();
  if (tid == 0) {
    double sum = s_sum[0];
#pragma unroll
    for (int w = 1; w < QW; ++w) sum += s_sum[w];
    if (ap) ap[b] = sum / (double)P;             // P == 0: 0 / 0, the mean of no term
    if (n_pos) n_pos[b] = P;
  }
  if (hits && tid < n_topk) {
    int h = 0;
#pragma unroll
    for (int w = 0; w < QW; ++w) h += s_hits[w][tid];
    hits[(int64_t)b * n_topk + tid] = h;
  }
}

// crit_attribute.py:64-68 on integers, in double: a clip without a positive divides by zero as the reference does
__device__ __forceinline__ double q_f1(int hit_i, int k, int P) {
  const double hit = hit_i == 0 ? 1e-3 : (double)hit_i;
  const double precision = hit / (double)k, recall = hit / (double)P;
  return 2.0 * precision * recall / (precision + recall);
}

// one workgroup; thread t owns the clips t, t + 1024, ...; the doubles by a scan in lane order, then the waves in wave order
__global__ __launch_bounds__(TT) void concept_totals_kernel(const double* ap, const int32_t* hits, const int32_t* n_pos, int B,
                                                            TopK topk, int n_topk, double* tot_d, int64_t* tot_i) {
  __shared__ double sd[16][QN + 1];
  __shared__ long long si[16][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a[QN + 1];
#pragma unroll
  for (int t = 0; t <= QN; ++t) a[t] = 0.0;
  long long clips = 0, empty = 0;
  for (int r = tid; r < B; r += TT) {
    const int P = n_pos[r];
#pragma unroll
    for (int t = 0; t < QN; ++t)
      if (t < n_topk) a[t] += q_f1(hits[(int64_t)r * n_topk + t], topk.k[t], P);
    a[QN] += ap[r];
    clips += 1;
    empty += P == 0 ? 1 : 0;
  }
#pragma unroll
  for (int t = 0; t <= QN; ++t) a[t] = care_wave_scan_total(a[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    clips += __shfl_xor(clips, o, 64);
    empty += __shfl_xor(empty, o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t <= QN; ++t) sd[wave][t] = a[t];
    si[wave][0] = clips;
    si[wave][1] = empty;
  }
  __syncthreads();
  if (tid <= n_topk) {                           // totals_d = (sum F1@k_0, .., sum F1@k_{n - 1}, sum AP)
    const int t = tid < n_topk ? tid : QN;
    double s = sd[0][t];
    for (int q = 1; q < 16; ++q) s += sd[q][t];
    tot_d[tid] += s;
  }
  if (tid == 64 || tid == 65) {
    const int k = tid - 64;
    long long s = 0;
    for (int q = 0; q < 16; ++q) s += si[q][k];
    tot_i[k] += s;
  }
}

inline bool q_mis4(const void* p) { return (((uintptr_t)p) & 3u) != 0; }

}  // namespace

extern "C" int care_concept_metrics(const float* preds, int64_t ldp, const float* labels, int64_t ldl, int B, int K,
                                    const int32_t* topk, int n_topk, double* ap, int32_t* hits, int32_t* n_pos,
                                    double* totals_d, int64_t* totals_i, void* stream) {
  if (!preds || !labels || B < 0 || K < 1 || n_topk < 0 || n_topk > QN || ldp < K || ldl < K) return CARE_EINVAL;
  if (n_topk > 0 && !topk) return CARE_EINVAL;
  if ((totals_d != nullptr) != (totals_i != nullptr)) return CARE_EINVAL;
  if (totals_d && (!ap || !n_pos || (n_topk > 0 && !hits))) return CARE_EINVAL;   // the totals are sums of the per-clip outputs
  TopK tk;
  for (int t = 0; t < QN; ++t) tk.k[t] = t < n_topk ? topk[t] : 1;
  for (int t = 0; t < n_topk; ++t)
    if (tk.k[t] < 1) return CARE_EINVAL;
  if (K > QK) return CARE_ESHAPE;
  for (int t = 0; t < n_topk; ++t)
    if (tk.k[t] > K) return CARE_ESHAPE;
  if (q_mis4(preds) || q_mis4(labels) || q_mis4(hits) || q_mis4(n_pos) ||
      !(care_aligned8(ap) && care_aligned8(totals_d) && care_aligned8(totals_i)))
    return CARE_EALIGN;
  if (B == 0) return 0;
  hipLaunchKernelGGL(concept_metrics_kernel, dim3(B), dim3(QT), 0, CST, preds, ldp, labels, ldl, K, tk, n_topk, ap, hits, n_pos);
  int rc = care_launch_status();
  if (rc != 0 || !totals_d) return rc;
  hipLaunchKernelGGL(concept_totals_kernel, dim3(1), dim3(TT), 0, CST, ap, hits, n_pos, B, tk, n_topk, totals_d, totals_i);
  return care_launch_status();
}
