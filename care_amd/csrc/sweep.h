// sweep.h - the chunked sweep under the streaming kernels of optim.hip (gradient norm, Adam) and interplay.hip (moving
// average, distillation loss and its gradient).  Every tensor is cut into chunks of 1024 elements (a small tensor is one
// short chunk), a grid of at most 2048 workgroups of 256 splits the chunks of a launch into contiguous ranges of equal
// length (+-1), and a workgroup walks its range.  A chunk whose pointers are 16-byte aligned moves as one float4 per lane
// and array (+ 0..3 tail scalars in a tensor's last chunk); any other chunk as scalars.  A list of tensors reaches its
// kernel BY VALUE in the arguments, N descriptors a launch.  No floating-point atomics: a workgroup's sum goes to a partial
// of its own (double), a second one-workgroup kernel adds the partials in index order.
//
// The host part is plain C++ with no HIP in it: the launch is a callable, so tools/micro/sweep_host_check.hip runs exactly
// this code under the host sanitizers with the launch stubbed out.
#pragma once
#include <stdint.h>
#include "../../include/care_hip.h"

constexpr int CARE_SWEEP_THREADS = 256;
constexpr int CARE_SWEEP_CHUNK = 1024;  // elements of a chunk: 256 lanes x one 16-byte access per array
static_assert(CARE_SWEEP_CHUNK == 4 * CARE_SWEEP_THREADS, "a chunk is one float4 per lane");

constexpr int64_t care_sweep_chunks(int64_t n) { return n / CARE_SWEEP_CHUNK + (n % CARE_SWEEP_CHUNK != 0); }

// workgroups (and partials) of a launch over `chunks` chunks
constexpr int care_sweep_grid(int64_t chunks) { return chunks < 1 ? 1 : chunks < 2048 ? (int)chunks : 2048; }

// What one launch gets, by value.  Tensor i owns the chunks start[i] .. start[i + 1] - 1 of the launch; an empty tensor
// owns none.  T is a descriptor with an int64_t n.
template <class T, int N>
struct care_sweep_pack {
  T t[N];
  int32_t start[N + 1];
  int32_t count;
};

// CARE_EINVAL / CARE_EALIGN / CARE_ESHAPE for a list no launch may see, else 0: per_tensor(descriptor) in index order, its
// first non-zero return wins; then no pack of N may have more chunks than a launch can number.
template <int N, class T, class Rule>
static inline int care_sweep_check(const T* ts, int count, Rule&& per_tensor) {
  if (count < 0 || (count > 0 && !ts)) return CARE_EINVAL;
  for (int i = 0; i < count; ++i) {
    const int bad = per_tensor(ts[i]);
    if (bad) return bad;
  }
  for (int i0 = 0; i0 < count; i0 += N) {
    int64_t chunks = 0;  // (each term is below 2^53 + 1 and a pack has at most 128 of them: no overflow)
    for (int i = i0; i < count && i < i0 + N; ++i) chunks += care_sweep_chunks(ts[i].n);
    if (chunks > 0x7fffffff) return CARE_ESHAPE;
  }
  return 0;
}

// launch(pack, chunks of the pack, index of the launch) for every N tensors of a CHECKED list; a non-zero return of the
// callable ends the walk and is handed on.  The unused tail of a pack is zero.
template <int N, class T, class Launch>
static inline int care_sweep_for_each_pack(const T* ts, int count, Launch&& launch) {
  int li = 0;
  for (int i0 = 0; i0 < count; i0 += N, ++li) {
    care_sweep_pack<T, N> pk = {};
    const int k = count - i0 < N ? count - i0 : N;
    int64_t c = 0;
    for (int i = 0; i < k; ++i) {
      pk.t[i] = ts[i0 + i];
      pk.start[i] = (int32_t)c;
      c += care_sweep_chunks(ts[i0 + i].n);
    }
    for (int i = k; i <= N; ++i) pk.start[i] = (int32_t)c;
    pk.count = k;
    const int rc = launch(pk, (int)c, li);
    if (rc != 0) return rc;
  }
  return 0;
}

// The rules of the two lists (here, not next to their kernels, so that the host check runs them and not a copy).
using care_opt_pack = care_sweep_pack<care_opt_tensor, CARE_OPT_PACK>;
using care_ema_pack = care_sweep_pack<care_ema_tensor, CARE_EMA_PACK>;

// care_grad_sqnorm / care_adam_step; *total = sum n
static inline int care_opt_check(const care_opt_tensor* ts, int count, int64_t* total) {
  int64_t sum = 0;
  const int bad = care_sweep_check<CARE_OPT_PACK>(ts, count, [&](const care_opt_tensor& d) -> int {
    if (!d.p || !d.g || !d.m || !d.v || d.n < 0) return CARE_EINVAL;
    if ((((uintptr_t)d.p) | ((uintptr_t)d.g) | ((uintptr_t)d.m) | ((uintptr_t)d.v)) & 3u) return CARE_EALIGN;
    if (d.n > INT64_MAX - sum) return CARE_ESHAPE;
    sum += d.n;
    return 0;
  });
  if (!bad && total) *total = sum;
  return bad;
}

// care_ema_step
static inline int care_ema_check(const care_ema_tensor* ts, int count) {
  return care_sweep_check<CARE_EMA_PACK>(ts, count, [](const care_ema_tensor& d) -> int {
    if (!d.t || !d.s || d.n < 0 || d.t == d.s) return CARE_EINVAL;
    if ((((uintptr_t)d.t) | ((uintptr_t)d.s)) & 3u) return CARE_EALIGN;
    return 0;
  });
}

#ifdef CARE_WAVE  // the device part, for the kernels (they come through care_common.h): helpers over callables, inlined

// the tensor that owns chunk ch of the pack: the last i with start[i] <= ch (an empty tensor never is)
template <class Pack>
__device__ __forceinline__ int care_sweep_owner(const Pack& pk, int ch) {
  int lo = 0, hi = pk.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pk.start[mid] <= ch) lo = mid; else hi = mid;
  }
  return lo;
}

// the chunks c0 .. c1 - 1 of this workgroup
template <class I>
__device__ __forceinline__ void care_sweep_range(I chunks, I& c0, I& c1) {
  c0 = (I)((int64_t)chunks * blockIdx.x / gridDim.x);
  c1 = (I)((int64_t)chunks * (blockIdx.x + 1) / gridDim.x);
}

// body(first element, elements) for every chunk of this workgroup out of ONE array of n elements
template <class Body>
__device__ __forceinline__ void care_sweep_array(int64_t n, Body&& body) {
  int64_t c0, c1;
  care_sweep_range(care_sweep_chunks(n), c0, c1);
  for (int64_t ch = c0; ch < c1; ++ch) {
    const int64_t e0 = ch * CARE_SWEEP_CHUNK;
    const int64_t left = n - e0;
    body(e0, left < CARE_SWEEP_CHUNK ? (int)left : CARE_SWEEP_CHUNK);
  }
}

// body(tensor, first element, elements) for every chunk of this workgroup out of a pack, the tensor index moving along
template <class Pack, class Body>
__device__ __forceinline__ void care_sweep_tensors(const Pack& pk, int chunks, Body&& body) {
  int c0, c1;
  care_sweep_range(chunks, c0, c1);
  if (c0 >= c1) return;
  int ti = care_sweep_owner(pk, c0);
  for (int ch = c0; ch < c1; ++ch) {
    while (pk.start[ti + 1] <= ch) ++ti;
    const int64_t e0 = (int64_t)(ch - pk.start[ti]) * CARE_SWEEP_CHUNK;
    const int64_t left = pk.t[ti].n - e0;
    body(ti, e0, left < CARE_SWEEP_CHUNK ? (int)left : CARE_SWEEP_CHUNK);
  }
}

// one chunk of len elements over the lanes: f4(i) takes the elements 4 i .. 4 i + 3 (vec: every pointer of the chunk is
// 16-byte aligned), f1(i) takes element i
template <class F4, class F1>
__device__ __forceinline__ void care_sweep_lanes(int len, bool vec, int tid, F4&& f4, F1&& f1) {
  if (vec) {
    const int n4 = len >> 2, tail = len & 3;
    if (tid < n4) f4(tid);
    if (tid < tail) f1(4 * n4 + tid);
  } else {
    for (int i = tid; i < len; i += CARE_SWEEP_THREADS) f1(i);
  }
}

// the sum of d over the workgroup, in thread 0 (sm: CARE_SWEEP_THREADS / 64 doubles of LDS); the waves meet in a fixed order
__device__ __forceinline__ double care_block_sum(double d, double* sm) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  if ((tid & 63) == 0) sm[tid >> 6] = d;
  __syncthreads();
  return tid == 0 ? (sm[0] + sm[1]) + (sm[2] + sm[3]) : 0.0;
}

// partials[0] + partials[1] + ... in thread 0 of ONE workgroup: lane t adds t, t + 256, ..., the lanes meet in a fixed order
__device__ __forceinline__ double care_partials_finish(const double* partials, int n, double* sm) {
  double d = 0.0;
  for (int i = threadIdx.x; i < n; i += CARE_SWEEP_THREADS) d += partials[i];
  return care_block_sum(d, sm);
}

#endif  // CARE_WAVE
