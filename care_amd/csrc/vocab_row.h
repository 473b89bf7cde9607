// vocab_row.h - one row of the [rows, V] fp32 logits under a workgroup of 256: the sweeps of the language loss (loss.hip) and
// of the advantage-weighted log-likelihood (reward.hip), written once.  A row starts at any 4-byte phase (ld = V = 10547 is
// odd): `head` = 0..3 scalars up to the next 16-byte boundary, n4 float4s, `tail` = 0..3 scalars; the (at most 6) scalars are
// "edge columns", one thread each.  The forward holds a row in registers between its two sweeps (NV4 > 0) or reads it again
// (NV4 == 0); the backward walks the row of the gradient, aligned on the STORE side.  A kernel keeps what is its own: what it
// gathers in the first sweep (a visitor), its epilogue, its gradient (a functor), which rows it skips.
//
// reward.hip compiles with floating-point contraction off and loss.hip with it on, and both must get the same bits out of
// this file: NOTHING here may have the shape a * b + c, and no fp pragma belongs here (it would reach the includer's code).
// What can be contracted stays in the callers' functors and epilogues.
#pragma once
#include "care_common.h"

constexpr int CARE_ROW_THREADS = 256;  // threads of a row workgroup (4 waves)

// x[0 .. V) as head scalars, n4 aligned float4s from x + head, tail scalars; ec = the edge column of this thread (-1: none):
// thread t < head owns x[t], the next `tail` threads the row's end
struct care_row_span {
  int head, n4, tail, ec;
};

__device__ __forceinline__ care_row_span care_row_span_of(const float* x, int V) {
  const int tid = threadIdx.x;
  care_row_span s;
  s.head = (int)((4u - (unsigned)(((uintptr_t)x >> 2) & 3u)) & 3u);
  if (s.head > V) s.head = V;
  s.n4 = (V - s.head) >> 2;
  s.tail = V - s.head - 4 * s.n4;
  int ec = -1;
  if (tid < s.head) ec = tid;
  else if (tid < s.head + s.tail) ec = s.head + 4 * s.n4 + (tid - s.head);
  s.ec = ec;
  return s;
}

// The four waves of a row workgroup meet through LDS, in wave order; every thread gets the result, and sm / si (4 elements)
// may be used again at once.
__device__ __forceinline__ float care_block_sum4(float v, float* sm) {
  v = care_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  const float t = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  return t;
}

__device__ __forceinline__ float care_block_max4(float v, float* sm) {
  v = care_wave_max(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  const float t = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  __syncthreads();
  return t;
}

// (best, bi) -> the largest value of the workgroup and its lowest column
__device__ __forceinline__ void care_block_argmax4(float& best, int& bi, float* sm, int* si) {
  care_wave_argmax(best, bi);
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  best = sm[0]; bi = si[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) care_argmax_take(best, bi, sm[w], si[w]);
  __syncthreads();
}

// A live row in the forward.  sweep() reads it once and shows every value to the kernel: edge(value, column) for the
// thread's edge scalar, then body(float4, its first column) for each of its float4s; sum_exp() is the second sweep.
template <int NV4>
struct care_row {
  care_row_span sp;
  const float4* xb;
  float ev;
  float4 v[NV4 > 0 ? NV4 : 1];

  template <class Edge, class Body>
  __device__ __forceinline__ void sweep(const float* x, int V, Edge&& edge, Body&& body) {
    const int tid = threadIdx.x;
    sp = care_row_span_of(x, V);
    xb = reinterpret_cast<const float4*>(x + sp.head);
    ev = 0.f;
    if (sp.ec >= 0) { ev = x[sp.ec]; edge(ev, sp.ec); }
    if (NV4 > 0) {
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        const int j = tid + i * CARE_ROW_THREADS;
        if (j < sp.n4) v[i] = xb[j];
      }
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        const int j = tid + i * CARE_ROW_THREADS;
        if (j < sp.n4) body(v[i], sp.head + 4 * j);
      }
    } else {
      for (int j = tid; j < sp.n4; j += CARE_ROW_THREADS) body(xb[j], sp.head + 4 * j);
    }
  }

  // this thread's part of sum exp(x - best): (a + b) + (c + d) per float4
  __device__ __forceinline__ float sum_exp(float best) const {
    const int tid = threadIdx.x;
    float s = 0.f;
    if (sp.ec >= 0) s += expf(ev - best);
    if (NV4 > 0) {
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        const int j = tid + i * CARE_ROW_THREADS;
        if (j < sp.n4) s += (expf(v[i].x - best) + expf(v[i].y - best)) + (expf(v[i].z - best) + expf(v[i].w - best));
      }
    } else {
      for (int j = tid; j < sp.n4; j += CARE_ROW_THREADS) {
        const float4 q = xb[j];
        s += (expf(q.x - best) + expf(q.y - best)) + (expf(q.z - best) + expf(q.w - best));
      }
    }
    return s;
  }
};

// A row d[0 .. V) of the gradient, sp = care_row_span_of(d, V): all zero ...
__device__ __forceinline__ void care_row_zero(float* d, const care_row_span& sp) {
  float4* db = reinterpret_cast<float4*>(d + sp.head);
  if (sp.ec >= 0) d[sp.ec] = 0.f;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = threadIdx.x; j < sp.n4; j += CARE_ROW_THREADS) db[j] = z;
}

// ... or d[c] = f(x[c], c).  The loads are float4s too when the logits row has the same 16-byte phase (always so when both
// tensors are contiguous with one leading dimension), four scalars otherwise.
template <class F>
__device__ __forceinline__ void care_row_map(const float* x, float* d, const care_row_span& sp, F&& f) {
  const int tid = threadIdx.x;
  float4* db = reinterpret_cast<float4*>(d + sp.head);
  if (sp.ec >= 0) d[sp.ec] = f(x[sp.ec], sp.ec);
  if (const bool same_phase = ((((uintptr_t)x) ^ ((uintptr_t)d)) & 15u) == 0) {
    const float4* xb = reinterpret_cast<const float4*>(x + sp.head);
#pragma unroll 4
    for (int j = tid; j < sp.n4; j += CARE_ROW_THREADS) {
      const float4 q = xb[j];
      const int c0 = sp.head + 4 * j;
      db[j] = make_float4(f(q.x, c0), f(q.y, c0 + 1), f(q.z, c0 + 2), f(q.w, c0 + 3));
    }
  } else {
    for (int j = tid; j < sp.n4; j += CARE_ROW_THREADS) {
      const int c0 = sp.head + 4 * j;
      db[j] = make_float4(f(x[c0], c0), f(x[c0 + 1], c0 + 1), f(x[c0 + 2], c0 + 2), f(x[c0 + 3], c0 + 3));
    }
  }
}

// The argument checks the entry points share, in their order.  `given`: every pointer of the entry point is there;
// own_shape / own_align: what only that entry point asks for a CARE_ESHAPE / CARE_EALIGN (true = fine).
// Forward: rows of [rows / rows_per_seq] sequences, sequence s at logits + s seq_stride, its row p at + p ld.
static inline int care_row_check_fwd(bool given, const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V,
                                     int rows, bool own_shape, bool own_align) {
  if (!given || rows <= 0 || V <= 0 || rows_per_seq <= 0) return CARE_EINVAL;
  if (ld < V || seq_stride < (int64_t)rows_per_seq * ld || !own_shape) return CARE_ESHAPE;
  if (((uintptr_t)logits & 3u) || !own_align) return CARE_EALIGN;
  return 0;
}

// Backward: dlogits has seq_rows >= rows_per_seq rows a sequence; *grid = its rows, one workgroup each.
static inline int care_row_check_bwd(bool given, const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V,
                                     const float* dlogits, int64_t ldd, int64_t dseq_stride, int seq_rows, int rows,
                                     bool own_shape, bool own_align, unsigned* grid) {
  if (!given || rows <= 0 || V <= 0 || rows_per_seq <= 0) return CARE_EINVAL;
  if (ld < V || ldd < V || seq_rows < rows_per_seq || rows % rows_per_seq != 0 || seq_stride < (int64_t)rows_per_seq * ld ||
      dseq_stride < (int64_t)seq_rows * ldd || !own_shape)
    return CARE_ESHAPE;
  if (((uintptr_t)logits & 3u) || ((uintptr_t)dlogits & 3u) || !own_align) return CARE_EALIGN;
  const int64_t g = (int64_t)(rows / rows_per_seq) * seq_rows;
  if (g > 0x7fffffff) return CARE_ESHAPE;
  *grid = (unsigned)g;
  return 0;
}
