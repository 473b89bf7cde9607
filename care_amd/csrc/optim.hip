// optim.hip - the optimiser step (include/care_hip.h, "The optimiser step"): clip_grad_norm_'s norm over all gradients and
// torch.optim.Adam's update of all parameters (models/Wrapper.py:316-386, train.py:128, care_amd/optim.py), each ONE sweep
// over every tensor of the list.  fp32 in both library variants.
//
// 32 B per element and step (norm: read g; update: read p, g, m, v, write p, m, v) and ~40 VALU operations: a streaming
// kernel.  The tensor list (55 tensors from 500 to 5.4 M elements in msrvtt_care) reaches the kernel BY VALUE in its
// arguments (sweep.h: CARE_OPT_PACK descriptors a launch) - gradients are fresh allocations every step, so a device-side
// table would be an upload per step.  The cut into chunks, the walk, the lanes of a chunk and the sums are sweep.h's.
#include "care_common.h"
#include "sweep.h"

namespace {

#define OST ((hipStream_t)stream)
constexpr int OT = CARE_SWEEP_THREADS;
static_assert(sizeof(care_opt_tensor) == 48 && sizeof(care_opt_pack) <= 3584, "the pack and the scalars fit the 4-KB argument block");

// partials[b] (+)= sum of g^2 over workgroup b's chunks.  first != 0: the launch that opens a list writes every
// partial (0 for a workgroup without chunks); the launches behind it add in stream order.
__global__ __launch_bounds__(OT) void grad_sqnorm_kernel(const care_opt_pack pk, int chunks, double* partials, int first) {
  __shared__ double sm[OT / 64];
  const int tid = threadIdx.x;
  float acc = 0.f;  // in float across the chunks; double from the shuffle upward
  care_sweep_tensors(pk, chunks, [&](int ti, int64_t e0, int len) {
    const float* g = pk.t[ti].g + e0;
    care_sweep_lanes(len, (((uintptr_t)g) & 15u) == 0, tid,
                     [&](int i) {
                       const float4 q = reinterpret_cast<const float4*>(g)[i];
                       acc += (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
                     },
                     [&](int i) { const float x = g[i]; acc += x * x; });
  });
  const double s = care_block_sum((double)acc, sm);
  if (tid == 0) partials[blockIdx.x] = first ? s : partials[blockIdx.x] + s;
}

// *norm = sqrt(partials[0] + partials[1] + ...)
__global__ __launch_bounds__(OT) void grad_norm_finish_kernel(const double* partials, int n, float* norm) {
  __shared__ double sm[OT / 64];
  const double s = care_partials_finish(partials, n, sm);
  if (threadIdx.x == 0) *norm = (float)sqrt(s);
}

struct adam_consts {
  float clip, wd, omb1, beta2, omb2, neg_step, bias2_sqrt, eps;
};

// torch/optim/adam.py, _single_tensor_adam: grad.add(param, alpha = wd); exp_avg.lerp_(grad, 1 - beta1);
// exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2); denom = exp_avg_sq.sqrt() / bias2_sqrt + eps;
// param.addcdiv_(exp_avg, denom, value = -step_size)
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const adam_consts& k) {
  g *= k.clip;
  if (k.wd != 0.f) g += k.wd * p;
  m += (g - m) * k.omb1;
  v = v * k.beta2 + k.omb2 * (g * g);
  p += k.neg_step * (m / (sqrtf(v) / k.bias2_sqrt + k.eps));
}

__global__ __launch_bounds__(OT) void adam_step_kernel(const care_opt_pack pk, int chunks, float omb1, float beta2, float omb2,
                                                       float eps, float bias2_sqrt, const float* norm, float max_norm) {
  const int tid = threadIdx.x;
  int c0, c1;
  care_sweep_range(chunks, c0, c1);
  if (c0 >= c1) return;  // ahead of the read of *norm, so that all arguments load in one batch before it
  adam_consts k;
  k.clip = 1.f;
  if (norm) {  // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays a NaN)
    const float q = max_norm / (*norm + 1e-6f);
    k.clip = q > 1.f ? 1.f : q;
  }
  k.omb1 = omb1; k.beta2 = beta2; k.omb2 = omb2; k.bias2_sqrt = bias2_sqrt; k.eps = eps;
  care_sweep_tensors(pk, chunks, [&](int ti, int64_t e0, int len) {
    float* p = pk.t[ti].p + e0;
    const float* g = pk.t[ti].g + e0;
    float* m = pk.t[ti].m + e0;
    float* v = pk.t[ti].v + e0;
    k.wd = pk.t[ti].weight_decay;
    k.neg_step = -pk.t[ti].step_size;
    care_sweep_lanes(len, ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15u) == 0, tid,
                     [&](int i) {
                       float4 P = reinterpret_cast<float4*>(p)[i];
                       const float4 G = reinterpret_cast<const float4*>(g)[i];
                       float4 M = reinterpret_cast<float4*>(m)[i];
                       float4 V = reinterpret_cast<float4*>(v)[i];
                       adam_one(P.x, G.x, M.x, V.x, k);
                       adam_one(P.y, G.y, M.y, V.y, k);
                       adam_one(P.z, G.z, M.z, V.z, k);
                       adam_one(P.w, G.w, M.w, V.w, k);
                       reinterpret_cast<float4*>(p)[i] = P;
                       reinterpret_cast<float4*>(m)[i] = M;
                       reinterpret_cast<float4*>(v)[i] = V;
                     },
                     [&](int i) {
                       float P = p[i], M = m[i], V = v[i];
                       adam_one(P, g[i], M, V, k);
                       p[i] = P; m[i] = M; v[i] = V;
                     });
  });
}

}  // namespace

extern "C" int care_grad_sqnorm_partials(int64_t total) { return care_sweep_grid(care_sweep_chunks(total)); }

extern "C" int care_grad_sqnorm(const care_opt_tensor* tensors, int count, double* partials, float* norm, void* stream) {
  if (!partials || !norm) return CARE_EINVAL;
  if ((((uintptr_t)partials) & 7u) || (((uintptr_t)norm) & 3u)) return CARE_EALIGN;
  int64_t total = 0;
  const int bad = care_opt_check(tensors, count, &total);
  if (bad) return bad;
  const int grid = care_grad_sqnorm_partials(total);
  if (count == 0) {  // one empty launch: every partial (there is one) = 0
    care_opt_pack pk = {};
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(OT), 0, OST, pk, 0, partials, 1);
  }
  const int rc = care_sweep_for_each_pack<CARE_OPT_PACK>(tensors, count, [&](const care_opt_pack& pk, int chunks, int li) {
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(OT), 0, OST, pk, chunks, partials, li == 0 ? 1 : 0);
    return care_launch_status();
  });
  if (rc) return rc;
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(OT), 0, OST, partials, grid, norm);
  return care_launch_status();
}

extern "C" int care_adam_step(const care_opt_tensor* tensors, int count, double beta1, double beta2, double eps, double bias2_sqrt,
                              const float* norm, double max_norm, void* stream) {
  if (norm && (((uintptr_t)norm) & 3u)) return CARE_EALIGN;
  const int bad = care_opt_check(tensors, count, nullptr);
  if (bad) return bad;
  if (count == 0) return 0;
  if (!(bias2_sqrt > 0.0)) return CARE_EINVAL;
  const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
  return care_sweep_for_each_pack<CARE_OPT_PACK>(tensors, count, [&](const care_opt_pack& pk, int chunks, int) {
    if (chunks == 0) return 0;
    hipLaunchKernelGGL(adam_step_kernel, dim3(care_sweep_grid(chunks)), dim3(OT), 0, OST, pk, chunks, omb1, b2, omb2, (float)eps,
                       (float)bias2_sqrt, norm, (float)max_norm);
    return care_launch_status();
  });
}
