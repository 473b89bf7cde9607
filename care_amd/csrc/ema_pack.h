// ema_pack.h - the HOST side of interplay.hip's care_ema_step: the argument checks and the packing of a host array of
// care_ema_tensor into the by-value kernel argument, CARE_EMA_PACK tensors per launch.  Plain C++ with no HIP in it: the
// launch is a callable, so tools/micro/ema_host_check.hip runs exactly this code under the host sanitizers with the
// launch stubbed out.
#pragma once
#include <stdint.h>
#include "../../include/care_hip.h"

constexpr int CARE_EMA_CHUNK = 1024;  // elements of a chunk: 256 lanes x one 16-byte access per array

// What one launch gets, by value (24 B a tensor + its first chunk: 3.5 KB of the 4 KB argument block).  Tensor i owns
// the chunks start[i] .. start[i + 1] - 1 of the launch; an empty tensor owns none.
struct care_ema_pack {
  care_ema_tensor t[CARE_EMA_PACK];
  int32_t start[CARE_EMA_PACK + 1];
  int32_t count;
};

static inline int64_t care_ema_chunks(int64_t n) { return n / CARE_EMA_CHUNK + (n % CARE_EMA_CHUNK != 0); }

// CARE_EINVAL / CARE_EALIGN / CARE_ESHAPE for a list no launch may see, else 0.
static inline int care_ema_check(const care_ema_tensor* ts, int count) {
  if (count < 0 || (count > 0 && !ts)) return CARE_EINVAL;
  for (int i = 0; i < count; ++i) {
    const care_ema_tensor& d = ts[i];
    if (!d.t || !d.s || d.n < 0 || d.t == d.s) return CARE_EINVAL;
    if ((((uintptr_t)d.t) | ((uintptr_t)d.s)) & 3u) return CARE_EALIGN;
  }
  for (int i0 = 0; i0 < count; i0 += CARE_EMA_PACK) {
    int64_t chunks = 0;   // (each term is below 2^53 and a pack has 128 of them: no overflow)
    for (int i = i0; i < count && i < i0 + CARE_EMA_PACK; ++i) chunks += care_ema_chunks(ts[i].n);
    if (chunks > 0x7fffffff) return CARE_ESHAPE;
  }
  return 0;
}

// launch(pack, chunks of the pack, index of the launch) for every CARE_EMA_PACK tensors of a CHECKED list; a non-zero
// return of the callable ends the walk and is handed on.  The unused tail of a pack is zero.
template <class Launch>
static inline int care_ema_for_each_pack(const care_ema_tensor* ts, int count, Launch&& launch) {
  int li = 0;
  for (int i0 = 0; i0 < count; i0 += CARE_EMA_PACK, ++li) {
    care_ema_pack pk = {};
    const int k = count - i0 < CARE_EMA_PACK ? count - i0 : CARE_EMA_PACK;
    int64_t c = 0;
    for (int i = 0; i < k; ++i) {
      pk.t[i] = ts[i0 + i];
      pk.start[i] = (int32_t)c;
      c += care_ema_chunks(ts[i0 + i].n);
    }
    for (int i = k; i <= CARE_EMA_PACK; ++i) pk.start[i] = (int32_t)c;
    pk.count = k;
    const int rc = launch(pk, (int)c, li);
    if (rc != 0) return rc;
  }
  return 0;
}
