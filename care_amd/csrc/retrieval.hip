// retrieval.hip - caption retrieval (include/care_hip.h, "Caption retrieval"; pretreatment/clip_retrieval.py:47-83, :175-176,
// :305-321; care_amd/retrieval.py): the `r` modality built on device from a bank of caption embeddings.  fp32 in both
// library variants.
//
// care_retrieval_topk is four launches and never holds the [B, M] scores:
//   scan    q [B, D] x bank [M, D]^T on v_mfma_f32_16x16x4_f32 straight from registers (no LDS, no barrier: a wave is a
//           workgroup).  Bank rows are the A operand, query rows the B operand, so a lane ends with 4 bank columns of ONE
//           query row per tile and the maximum over the eligible columns of a 16-column group is 3 in-lane maxima and two
//           lane exchanges.  Out: gmax [B, groups].  Up to 16 rows a wave owns one group (8141 waves over a 130 K bank:
//           bound by the bank's bytes, 8 blocks of 16 k in flight per lane); from 33 rows 4 groups x 4 row tiles (16
//           independent accumulators, 64 MFMAs per 8 loads: bound by the matrix pipe).
//   groups  per row the topk groups by (maximum descending, group ascending): the topk-th largest ordered bit pattern found
//           bit by bit, then an index-ordered compaction.  The topk columns of a row lie in these groups: a column outside
//           them has topk groups ranked before its own, each with a column ranked before it.
//   rescore one wave per (row, chosen group): the group's 16 scores once more, the same operands to the same MFMAs in the
//           same order as the scan - bit-identical - and the eligibility once more; out: 64-bit keys (ordered score, ~column).
//   rank    per row a bitonic sort of the <= 16 topk keys in LDS, a thread per key; the first topk are the answer.
//
// One summation order for every (row, column): k in blocks of 16, within a block MFMA i takes k = 4 g + i from the lane
// group g.  It depends on nothing but D, so a bank row scores the same in every scan form, tile position and batch.
#include "care_common.h"
#include "retrieval_plan.h"

namespace {

#define RST ((hipStream_t)stream)
constexpr unsigned KEY_NEG_INF = 0x007FFFFFu;   // retr_ord(-inf): every finite score orders above it

// fp32 -> a uint32 that orders like the float
__device__ __forceinline__ unsigned retr_ord(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float retr_unord(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct RetrArgs {
  const float* q; const float* bank;
  int B, M, D, topk;
  const int32_t* start; const int32_t* end; const int32_t* first; const int32_t* prev; const int32_t* orig;
  float* gmax; int32_t* sel; int32_t* nsel; unsigned long long* cand;
  int groups, group_stride, row_blocks, sort_n;
  int64_t* ids; float* scores; int32_t* count;
};

// column j (its group links pj = prev[j], fj = first[j]; pj = -1 without `unique`) for a row with the own range [s, e)
__device__ __forceinline__ bool retr_eligible(int j, int M, int s, int e, int pj, int fj) {
  return j < M && !(j >= s && j < e) && (pj < 0 || (fj >= s && pj < e));
}

template <int BT, int QT, int P>
__global__ __launch_bounds__(64) void retr_scan_kernel(const RetrArgs p) {
  const int lane = threadIdx.x, fr = lane & 15, fg = lane >> 4;
  const int cb = blockIdx.x / p.row_blocks, rb = blockIdx.x % p.row_blocks;
  const int col0 = cb * 16 * BT, row0 = rb * 16 * QT;
  // (rows / columns past B / M are clamped: their products are never kept)
  const float* a[BT];
  const float* b[QT];
#pragma unroll
  for (int t = 0; t < BT; ++t) a[t] = p.bank + (int64_t)min(col0 + t * 16 + fr, p.M - 1) * p.D + fg * 4;
#pragma unroll
  for (int t = 0; t < QT; ++t) b[t] = p.q + (int64_t)min(row0 + t * 16 + fr, p.B - 1) * p.D + fg * 4;
  const int nb = p.D / 16;
  f32x4 ra[P][BT], rq[P][QT];
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int blk = min(u, nb - 1);
#pragma unroll
    for (int t = 0; t < BT; ++t) ra[u][t] = *reinterpret_cast<const f32x4*>(a[t] + blk * 16);
#pragma unroll
    for (int t = 0; t < QT; ++t) rq[u][t] = *reinterpret_cast<const f32x4*>(b[t] + blk * 16);
  }
  f32x4 acc[BT][QT];
#pragma unroll
  for (int t = 0; t < BT; ++t)
#pragma unroll
    for (int s = 0; s < QT; ++s) acc[t][s] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nb; kb += P) {
#pragma unroll
    for (int u = 0; u < P; ++u) {
      if (kb + u < nb) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < BT; ++t)
#pragma unroll
            for (int s = 0; s < QT; ++s) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[u][t][i], rq[u][s][i], acc[t][s], 0, 0, 0);
      }
      const int nxt = min(kb + u + P, nb - 1);   // unconditional refill of the slot just used (the tail re-reads the last block)
#pragma unroll
      for (int t = 0; t < BT; ++t) ra[u][t] = *reinterpret_cast<const f32x4*>(a[t] + nxt * 16);
#pragma unroll
      for (int t = 0; t < QT; ++t) rq[u][t] = *reinterpret_cast<const f32x4*>(b[t] + nxt * 16);
    }
  }
  // the lane holds, per tile pair, the columns col0 + 16 t + 4 fg + r (r = 0..3) of the row row0 + 16 s + fr
  int rs[QT], re[QT];
#pragma unroll
  for (int s = 0; s < QT; ++s) {
    const int row = min(row0 + s * 16 + fr, p.B - 1);
    rs[s] = p.start ? p.start[row] : 0;
    re[s] = p.start ? p.end[row] : 0;
  }
  float gm[QT][BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    const int j0 = col0 + t * 16 + fg * 4;
    int pj[4], fj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jc = min(j0 + r, p.M - 1);
      pj[r] = p.prev ? p.prev[jc] : -1;
      fj[r] = p.prev ? p.first[jc] : 0;
    }
#pragma unroll
    for (int s = 0; s < QT; ++s) {
      float m = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (retr_eligible(j0 + r, p.M, rs[s], re[s], pj[r], fj[r])) m = fmaxf(m, acc[t][s][r]);
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      gm[s][t] = m;
    }
  }
  if (fg != 0) return;
#pragma unroll
  for (int s = 0; s < QT; ++s) {
    const int row = row0 + s * 16 + fr;
    if (row >= p.B) continue;
    float* out = p.gmax + (int64_t)row * p.group_stride + cb * BT;   // (cb BT + t < group_stride = 4 ceil(M / 64) for every form)
    if constexpr (BT == 4) {
      *reinterpret_cast<f32x4*>(out) = f32x4{gm[s][0], gm[s][1], gm[s][2], gm[s][3]};
    } else {
#pragma unroll
      for (int t = 0; t < BT; ++t) out[t] = gm[s][t];
    }
  }
}

// sel [b, 0 .. nsel[b]) = the min(topk, groups with an eligible column) best groups of row b by (maximum descending, group
// ascending), in no particular order.  The K-th largest key is built bit by bit from the top - 32 rounds of "how many keys
// are >= the candidate" over keys held in registers (8 a thread: 8192 groups, a 131 K bank; the rest is re-read) - because
// scores of unit vectors share their leading bits and a histogram's atomics would all meet on one bin.
constexpr int GT = 1024;
__global__ __launch_bounds__(GT) void retr_groups_kernel(const RetrArgs p) {
  __shared__ unsigned cnt[3];
  __shared__ unsigned wt[GT / 64];
  __shared__ unsigned s_cnt;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, n = p.groups;
  const float* gm = p.gmax + (int64_t)b * p.group_stride;
  int32_t* sel = p.sel + (int64_t)b * p.topk;
  unsigned kv[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int i = tid + GT * t;
    kv[t] = i < n ? retr_ord(gm[i]) : 0u;           // (0 is below every threshold asked for)
  }
  if (tid < 3) cnt[tid] = 0;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int round = 0;
  // the number of keys >= thr (thr >= 1); every thread calls it.  Round r adds into cnt[r % 3] and clears cnt[(r + 1) % 3],
  // which was last read two barriers ago
  auto count_ge = [&](unsigned thr) -> unsigned {
    unsigned c = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) c += kv[t] >= thr;
    for (int i = tid + 8 * GT; i < n; i += GT) c += retr_ord(gm[i]) >= thr;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    const int slot = round % 3;
    if (tid == 0) cnt[(round + 1) % 3] = 0;
    if (lane == 0 && c) atomicAdd(&cnt[slot], c);
    __syncthreads();
    ++round;
    return cnt[slot];
  };
  const unsigned K = min((unsigned)p.topk, count_ge(KEY_NEG_INF + 1u));
  if (tid == 0) p.nsel[b] = (int)K;
  if (K == 0) return;
  unsigned T = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cand = T | (1u << bit);
    if (count_ge(cand) >= K) T = cand;
  }
  const unsigned ngt = T == 0xFFFFFFFFu ? 0u : count_ge(T + 1u);   // (< K)
  const unsigned take_eq = K - ngt;
  // every group above T, and of those at T the `take_eq` lowest
  unsigned eq_base = 0;
  for (int c0 = 0; c0 < n; c0 += GT) {
    const int i = c0 + tid;
    const unsigned key = i < n ? retr_ord(gm[i]) : 0u;
    if (key > T) {                                        // (exactly ngt of them: slots 0 .. ngt - 1)
      const unsigned slot = atomicAdd(&s_cnt, 1u);
      if (slot < ngt) sel[slot] = i;
    }
    const bool eq = key == T;
    const unsigned long long bal = __ballot(eq);
    if (lane == 0) wt[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned base = eq_base, all = 0;
#pragma unroll
    for (int x = 0; x < GT / 64; ++x) {
      base += x < w ? wt[x] : 0u;
      all += wt[x];
    }
    const unsigned rank = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    if (eq && rank < take_eq) sel[ngt + rank] = i;
    eq_base += all;
    __syncthreads();
  }
}

// cand [b, s, 0..15] = the keys of the 16 columns of row b's s-th chosen group (0: not eligible / no such group)
template <int P>
__global__ __launch_bounds__(64) void retr_rescore_kernel(const RetrArgs p) {
  const int lane = threadIdx.x, fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.x / p.topk, s = blockIdx.x % p.topk;
  unsigned long long* out = p.cand + ((int64_t)b * p.topk + s) * 16;
  if (s >= p.nsel[b]) {
    if (lane < 16) out[lane] = 0ull;
    return;
  }
  const int col0 = min(max(p.sel[(int64_t)b * p.topk + s], 0), p.groups - 1) * 16;
  const float* a = p.bank + (int64_t)min(col0 + fr, p.M - 1) * p.D + fg * 4;
  const float* q = p.q + (int64_t)b * p.D + fg * 4;     // the row in every column of the B operand
  const int nb = p.D / 16;
  f32x4 ra[P], rq[P];
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int blk = min(u, nb - 1);
    ra[u] = *reinterpret_cast<const f32x4*>(a + blk * 16);
    rq[u] = *reinterpret_cast<const f32x4*>(q + blk * 16);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nb; kb += P) {
#pragma unroll
    for (int u = 0; u < P; ++u) {
      if (kb + u < nb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[u][i], rq[u][i], acc, 0, 0, 0);
      }
      const int nxt = min(kb + u + P, nb - 1);
      ra[u] = *reinterpret_cast<const f32x4*>(a + nxt * 16);
      rq[u] = *reinterpret_cast<const f32x4*>(q + nxt * 16);
    }
  }
  if (fr != 0) return;
  const int rs = p.start ? p.start[b] : 0, re = p.start ? p.end[b] : 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = col0 + fg * 4 + r, jc = min(j, p.M - 1);
    const int pj = p.prev ? p.prev[jc] : -1, fj = p.prev ? p.first[jc] : 0;
    out[fg * 4 + r] = retr_eligible(j, p.M, rs, re, pj, fj)
                          ? (((unsigned long long)retr_ord(acc[r])) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j)
                          : 0ull;
  }
}

__global__ __launch_bounds__(1024) void retr_rank_kernel(const RetrArgs p) {
  __shared__ unsigned long long keys[16 * CARE_RETR_MAX_TOPK];
  const int tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x, N = p.sort_n;
  const int have = p.nsel[b] * 16;
  const unsigned long long* cand = p.cand + (int64_t)b * p.topk * 16;
  for (int i = tid; i < N; i += nt) keys[i] = i < have ? cand[i] : 0ull;
  __syncthreads();
  // bitonic, descending: a larger key is a larger score or, at the same score, a lower column
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < N; i += nt) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long u = keys[i], v = keys[x];
          if (((i & k) == 0) ? (u < v) : (u > v)) { keys[i] = v; keys[x] = u; }
        }
      }
      __syncthreads();
    }
  for (int t = tid; t < p.topk; t += nt) {
    const unsigned long long key = keys[t];   // (topk <= 16 topk <= N)
    const int64_t o = (int64_t)b * p.topk + t;
    if (key != 0ull) {
      const unsigned j = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
      p.ids[o] = p.orig ? (int64_t)p.orig[j] : (int64_t)j;
      p.scores[o] = retr_unord((unsigned)(key >> 32));
      if (t + 1 == p.topk || keys[t + 1] == 0ull) p.count[b] = t + 1;
    } else {
      p.ids[o] = -1;
      p.scores[o] = -INFINITY;
      if (t == 0) p.count[b] = 0;
    }
  }
}

// one wave per row: the row in registers (D / 4 <= 256 float4: up to 4 a lane), its sum of squares lane by lane in element
// order and then through the wave in a fixed order
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int M, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float4* src = reinterpret_cast<const float4*>(x + row * D);
  float4* dst = reinterpret_cast<float4*>(y + row * D);
  const int n4 = D / 4;
  float4 v[4];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = lane + 64 * t;
    v[t] = c < n4 ? src[c] : float4{0.f, 0.f, 0.f, 0.f};
    ss += v[t].x * v[t].x + v[t].y * v[t].y + v[t].z * v[t].z + v[t].w * v[t].w;
  }
  ss = care_wave_sum(ss);
  const float nrm = sqrtf(ss);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = lane + 64 * t;
    if (c < n4) dst[c] = float4{v[t].x / nrm, v[t].y / nrm, v[t].z / nrm, v[t].w / nrm};
  }
}

// one workgroup per clip: thread t owns the elements t, t + 256, ... (D <= 1024: up to 4), sums them over the frames in
// frame order, divides by n; the squares meet in a fixed order
__global__ __launch_bounds__(256) void retr_query_kernel(const float* __restrict__ frames, float* __restrict__ q, int n, int D) {
  __shared__ float sm[4];
  const int tid = threadIdx.x;
  const float* src = frames + (int64_t)blockIdx.x * n * D;
  float m[4];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int d = tid + 256 * t;
    float s = 0.f;
    if (d < D)
      for (int f = 0; f < n; ++f) s += src[(int64_t)f * D + d];
    m[t] = s / (float)n;
    ss += m[t] * m[t];
  }
  ss = care_wave_sum(ss);
  if ((tid & 63) == 0) sm[tid >> 6] = ss;
  __syncthreads();
  const float nrm = sqrtf((sm[0] + sm[1]) + (sm[2] + sm[3]));
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int d = tid + 256 * t;
    if (d < D) q[(int64_t)blockIdx.x * D + d] = m[t] / nrm;
  }
}

__global__ __launch_bounds__(256) void retr_gather_kernel(const float* __restrict__ table, int rows, int De, const int64_t* __restrict__ ids,
                                                          float* __restrict__ out) {
  const int64_t id = ids[blockIdx.x];
  const bool live = id >= 0 && id < rows;
  const float4* src = reinterpret_cast<const float4*>(table + (live ? id : 0) * De);
  float4* dst = reinterpret_cast<float4*>(out + (int64_t)blockIdx.x * De);
  for (int c = threadIdx.x; c < De / 4; c += 256) dst[c] = live ? src[c] : float4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace

extern "C" int care_l2_normalize_rows(const float* x, float* y, int M, int D, void* stream) {
  const int bad = care_l2_normalize_rows_check(x, y, M, D);
  if (bad) return bad;
  hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, RST, x, y, M, D);
  return care_launch_status();
}

extern "C" int care_retrieval_query(const float* frames, float* q, int B, int n, int D, void* stream) {
  const int bad = care_retrieval_query_check(frames, q, B, n, D);
  if (bad) return bad;
  hipLaunchKernelGGL(retr_query_kernel, dim3(B), dim3(256), 0, RST, frames, q, n, D);
  return care_launch_status();
}

extern "C" int64_t care_retrieval_scratch(int B, int M, int topk) {
  care_retrieval_plan pl;
  return care_retrieval_make_plan(B, M, topk, &pl) ? -1 : pl.bytes;
}

extern "C" int care_retrieval_topk(const float* q, const float* bank, int B, int M, int D, int topk, const int32_t* start,
                                   const int32_t* end, const int32_t* first, const int32_t* prev, const int32_t* orig,
                                   int64_t* ids, float* scores, int32_t* count, void* scratch, int64_t scratch_bytes, void* stream) {
  care_retrieval_plan pl;
  const int bad = care_retrieval_topk_check(q, bank, B, M, D, topk, start, end, first, prev, orig, ids, scores, count, scratch,
                                            scratch_bytes, &pl);
  if (bad) return bad;
  unsigned char* sc = static_cast<unsigned char*>(scratch);
  RetrArgs p;
  p.q = q; p.bank = bank; p.B = B; p.M = M; p.D = D; p.topk = topk;
  p.start = start; p.end = end; p.first = first; p.prev = prev; p.orig = orig;
  p.gmax = reinterpret_cast<float*>(sc + pl.off_gmax);
  p.sel = reinterpret_cast<int32_t*>(sc + pl.off_sel);
  p.nsel = reinterpret_cast<int32_t*>(sc + pl.off_nsel);
  p.cand = reinterpret_cast<unsigned long long*>(sc + pl.off_cand);
  p.groups = pl.groups; p.group_stride = pl.group_stride; p.row_blocks = pl.row_blocks; p.sort_n = pl.sort_n;
  p.ids = ids; p.scores = scores; p.count = count;
  const dim3 grid((unsigned)(pl.col_blocks * pl.row_blocks)), wave(64);
  if (pl.bt == 1) hipLaunchKernelGGL((retr_scan_kernel<1, 1, 8>), grid, wave, 0, RST, p);
  else if (pl.bt == 2) hipLaunchKernelGGL((retr_scan_kernel<2, 2, 4>), grid, wave, 0, RST, p);
  else hipLaunchKernelGGL((retr_scan_kernel<4, 4, 2>), grid, wave, 0, RST, p);
  int rc = care_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(retr_groups_kernel, dim3(B), dim3(GT), 0, RST, p);
  if ((rc = care_launch_status())) return rc;
  hipLaunchKernelGGL((retr_rescore_kernel<8>), dim3((unsigned)(B * topk)), wave, 0, RST, p);
  if ((rc = care_launch_status())) return rc;
  hipLaunchKernelGGL(retr_rank_kernel, dim3(B), dim3(pl.sort_n < 128 ? 64 : pl.sort_n > 1024 ? 1024 : pl.sort_n), 0, RST, p);
  return care_launch_status();
}

extern "C" int care_retrieval_gather(const float* table, int rows, int De, const int64_t* ids, int n, float* out, void* stream) {
  const int bad = care_retrieval_gather_check(table, rows, De, ids, n, out);
  if (bad) return bad;
  hipLaunchKernelGGL(retr_gather_kernel, dim3(n), dim3(256), 0, RST, table, rows, De, ids, out);
  return care_launch_status();
}
