// interplay.hip - the mean-teacher step (include/care_hip.h, "The mean-teacher step"; models/Wrapper.py:550-614,
// care_amd/interplay.py): the exponential moving average of every teacher parameter towards the student's as ONE sweep
// over the tensor list, and the distillation term mean((a - b)^2) over two logit tensors with its gradient.  fp32 in both
// library variants.
//
// All three are streaming kernels: 12 B per element for the average (read t, s, write t), 8 B for the loss (read a, b),
// 12 B for its gradient (read a, b, write da) and a handful of VALU operations.  The tensor list of the average reaches its
// kernel BY VALUE in the arguments (sweep.h: CARE_EMA_PACK descriptors a launch); the cut into chunks, the walk, the lanes
// of a chunk and the sums are sweep.h's.  The loss kernels cut ONE array the same way; its base may sit at any 4-byte
// phase (a row of logits is V = 10547 floats), so 0..3 scalars are peeled up to the 16-byte boundary and the chunks
// start there.
#include "care_common.h"
#include "sweep.h"

namespace {

#define IST ((hipStream_t)stream)
constexpr int IT = CARE_SWEEP_THREADS;
static_assert(sizeof(care_ema_tensor) == 24 && sizeof(care_ema_pack) <= 3840, "the pack and the scalars fit the 4-KB argument block");

// torch._foreach_mul_(t, w); torch._foreach_add_(t, torch._foreach_mul(s, 1 - w)): three roundings, never an FMA.
// (__fmul_rn / __fadd_rn are plain operators in their header, which the compiler contracts by default: the operators
// are written out here, under a pragma that keeps the two products and the sum apart.)
__device__ __forceinline__ float ema_one(float t, float s, float w, float omw) {
#pragma clang fp contract(off)
  const float a = t * w;
  const float b = s * omw;
  return a + b;
}

__global__ __launch_bounds__(IT) void ema_step_kernel(const care_ema_pack pk, int chunks, float w, float omw) {
  const int tid = threadIdx.x;
  care_sweep_tensors(pk, chunks, [&](int ti, int64_t e0, int len) {
    float* t = pk.t[ti].t + e0;
    const float* s = pk.t[ti].s + e0;
    care_sweep_lanes(len, ((((uintptr_t)t) | ((uintptr_t)s)) & 15u) == 0, tid,
                     [&](int i) {
                       float4 T = reinterpret_cast<float4*>(t)[i];
                       const float4 S = reinterpret_cast<const float4*>(s)[i];
                       T.x = ema_one(T.x, S.x, w, omw);
                       T.y = ema_one(T.y, S.y, w, omw);
                       T.z = ema_one(T.z, S.z, w, omw);
                       T.w = ema_one(T.w, S.w, w, omw);
                       reinterpret_cast<float4*>(t)[i] = T;
                     },
                     [&](int i) { t[i] = ema_one(t[i], s[i], w, omw); });
  });
}

// How one array of n floats at `base` is walked: `head` scalars up to the 16-byte boundary (all n when the arrays of a
// call do not share a phase: `vec` = false), then the chunks of the n - head behind them.
struct mse_walk {
  int64_t head;
  bool vec;
};

__device__ __forceinline__ mse_walk mse_plan(uintptr_t a, uintptr_t others_xor, int64_t n) {
  mse_walk wk;
  wk.vec = (others_xor & 15u) == 0;
  if (wk.vec) {
    const int64_t h = (int64_t)(((16u - (unsigned)(a & 15u)) & 15u) >> 2);
    wk.head = h < n ? h : n;
  } else {
    wk.head = 0;
  }
  return wk;
}

__device__ __forceinline__ void mse_acc(double& acc, float a, float b) {
  const double d = (double)(a - b);   // the difference in fp32, as torch takes it
  acc += d * d;
}

// partials[w] = sum over workgroup w's chunks of (a - b)^2, in double from the lane upward (0 for a workgroup without
// chunks; workgroup 0 takes the peeled head too, before its chunks)
__global__ __launch_bounds__(IT) void mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                         double* __restrict__ partials) {
  __shared__ double sm[IT / 64];
  const int tid = threadIdx.x;
  const mse_walk wk = mse_plan((uintptr_t)a, ((uintptr_t)a) ^ ((uintptr_t)b), n);
  double acc = 0.0;
  if (blockIdx.x == 0 && tid < wk.head) mse_acc(acc, a[tid], b[tid]);
  care_sweep_array(n - wk.head, [&](int64_t e0, int len) {
    const float* A = a + wk.head + e0;
    const float* B = b + wk.head + e0;
    care_sweep_lanes(len, wk.vec, tid,
                     [&](int i) {
                       const float4 x = reinterpret_cast<const float4*>(A)[i];
                       const float4 y = reinterpret_cast<const float4*>(B)[i];
                       mse_acc(acc, x.x, y.x);
                       mse_acc(acc, x.y, y.y);
                       mse_acc(acc, x.z, y.z);
                       mse_acc(acc, x.w, y.w);
                     },
                     [&](int i) { mse_acc(acc, A[i], B[i]); });
  });
  const double s = care_block_sum(acc, sm);
  if (tid == 0) partials[blockIdx.x] = s;
}

// *loss = (float)((partials[0] + partials[1] + ...) / n)
__global__ __launch_bounds__(IT) void mse_finish_kernel(const double* partials, int count, int64_t n, float* loss) {
  __shared__ double sm[IT / 64];
  const double s = care_partials_finish(partials, count, sm);
  if (threadIdx.x == 0) *loss = (float)(s / (double)n);
}

__device__ __forceinline__ float mse_grad_one(float a, float b, float c) {
#pragma clang fp contract(off)
  const float d = a - b;
  return d * c;
}

__global__ __launch_bounds__(IT) void mse_bwd_kernel(const float* a, const float* b, int64_t n, const float* __restrict__ g, float* da) {
  const int tid = threadIdx.x;
  const float c = (float)(2.0 * (double)*g / (double)n);
  const mse_walk wk = mse_plan((uintptr_t)a, (((uintptr_t)a) ^ ((uintptr_t)b)) | (((uintptr_t)a) ^ ((uintptr_t)da)), n);
  if (blockIdx.x == 0 && tid < wk.head) da[tid] = mse_grad_one(a[tid], b[tid], c);
  care_sweep_array(n - wk.head, [&](int64_t e0, int len) {
    const float* A = a + wk.head + e0;
    const float* B = b + wk.head + e0;
    float* D = da + wk.head + e0;
    care_sweep_lanes(len, wk.vec, tid,
                     [&](int i) {
                       const float4 x = reinterpret_cast<const float4*>(A)[i];
                       const float4 y = reinterpret_cast<const float4*>(B)[i];
                       float4 r;
                       r.x = mse_grad_one(x.x, y.x, c);
                       r.y = mse_grad_one(x.y, y.y, c);
                       r.z = mse_grad_one(x.z, y.z, c);
                       r.w = mse_grad_one(x.w, y.w, c);
                       reinterpret_cast<float4*>(D)[i] = r;
                     },
                     [&](int i) { D[i] = mse_grad_one(A[i], B[i], c); });
  });
}

}  // namespace

extern "C" int care_ema_step(const care_ema_tensor* tensors, int count, double w, double one_minus_w, void* stream) {
  const int bad = care_ema_check(tensors, count);
  if (bad) return bad;
  if (count == 0) return 0;
  const float wf = (float)w, omw = (float)one_minus_w;
  return care_sweep_for_each_pack<CARE_EMA_PACK>(tensors, count, [&](const care_ema_pack& pk, int chunks, int) {
    if (chunks == 0) return 0;
    hipLaunchKernelGGL(ema_step_kernel, dim3(care_sweep_grid(chunks)), dim3(IT), 0, IST, pk, chunks, wf, omw);
    return care_launch_status();
  });
}

extern "C" int care_mse_partials(int64_t n) { return care_sweep_grid(care_sweep_chunks(n)); }

extern "C" int care_mse_fwd(const float* a, const float* b, int64_t n, double* partials, float* loss, void* stream) {
  if (!a || !b || !partials || !loss || n <= 0) return CARE_EINVAL;
  if (((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)loss)) & 3u) || (((uintptr_t)partials) & 7u)) return CARE_EALIGN;
  const int grid = care_mse_partials(n);
  hipLaunchKernelGGL(mse_partial_kernel, dim3(grid), dim3(IT), 0, IST, a, b, n, partials);
  int rc = care_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(IT), 0, IST, partials, grid, n, loss);
  return care_launch_status();
}

extern "C" int care_mse_bwd(const float* a, const float* b, int64_t n, const float* g, float* da, void* stream) {
  if (!a || !b || !g || !da || n <= 0) return CARE_EINVAL;
  if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)g) | ((uintptr_t)da)) & 3u) return CARE_EALIGN;
  hipLaunchKernelGGL(mse_bwd_kernel, dim3(care_mse_partials(n)), dim3(IT), 0, IST, a, b, n, g, da);
  return care_launch_status();
}
