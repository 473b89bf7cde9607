// optim_pack.h - the HOST side of optim.hip: the argument checks of care_grad_sqnorm / care_adam_step and the packing of
// a host array of care_opt_tensor into the by-value kernel argument, CARE_OPT_PACK tensors per launch.  Plain C++ with no
// HIP in it: the launch is a callable, so tools/micro/optim_host_check.cpp runs exactly this code under the host
// sanitizers with the launch stubbed out.
#pragma once
#include <stdint.h>
#include "../../include/care_hip.h"

constexpr int CARE_OPT_CHUNK = 1024;  // elements of a chunk: 256 lanes x one 16-byte access per array

// What one launch gets, by value (48 B a tensor + its first chunk: 3.3 KB of the 4 KB argument block).  Tensor i owns
// the chunks start[i] .. start[i + 1] - 1 of the launch; an empty tensor owns none.
struct care_opt_pack {
  care_opt_tensor t[CARE_OPT_PACK];
  int32_t start[CARE_OPT_PACK + 1];
  int32_t count;
};

static inline int64_t care_opt_chunks(int64_t n) { return (n + CARE_OPT_CHUNK - 1) / CARE_OPT_CHUNK; }

// CARE_EINVAL / CARE_EALIGN / CARE_ESHAPE for a list no launch may see, else 0; *total = sum n.
static inline int care_opt_check(const care_opt_tensor* ts, int count, int64_t* total) {
  if (count < 0 || (count > 0 && !ts)) return CARE_EINVAL;
  int64_t sum = 0;
  for (int i = 0; i < count; ++i) {
    const care_opt_tensor& d = ts[i];
    if (!d.p || !d.g || !d.m || !d.v || d.n < 0) return CARE_EINVAL;
    if ((((uintptr_t)d.p) | ((uintptr_t)d.g) | ((uintptr_t)d.m) | ((uintptr_t)d.v)) & 3u) return CARE_EALIGN;
    if (d.n > INT64_MAX - sum) return CARE_ESHAPE;
    sum += d.n;
  }
  for (int i0 = 0; i0 < count; i0 += CARE_OPT_PACK) {
    int64_t chunks = 0;
    for (int i = i0; i < count && i < i0 + CARE_OPT_PACK; ++i) chunks += care_opt_chunks(ts[i].n);
    if (chunks > 0x7fffffff) return CARE_ESHAPE;
  }
  if (total) *total = sum;
  return 0;
}

// launch(pack, chunks of the pack, index of the launch) for every CARE_OPT_PACK tensors of a CHECKED list; a non-zero
// return of the callable ends the walk and is handed on.  The unused tail of a pack is zero.
template <class Launch>
static inline int care_opt_for_each_pack(const care_opt_tensor* ts, int count, Launch&& launch) {
  int li = 0;
  for (int i0 = 0; i0 < count; i0 += CARE_OPT_PACK, ++li) {
    care_opt_pack pk = {};
    const int k = count - i0 < CARE_OPT_PACK ? count - i0 : CARE_OPT_PACK;
    int64_t c = 0;
    for (int i = 0; i < k; ++i) {
      pk.t[i] = ts[i0 + i];
      pk.start[i] = (int32_t)c;
      c += care_opt_chunks(ts[i0 + i].n);
    }
    for (int i = k; i <= CARE_OPT_PACK; ++i) pk.start[i] = (int32_t)c;
    pk.count = k;
    const int rc = launch(pk, (int)c, li);
    if (rc != 0) return rc;
  }
  return 0;
}

static inline int care_opt_partials(int64_t total) {
  if (total <= 0) return 1;
  const int64_t c = care_opt_chunks(total);
  return (int)(c < 2048 ? c : 2048);
}
