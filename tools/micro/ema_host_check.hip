// ema_host_check.hip - the host launcher of care_ema_step (csrc/ema_pack.h: argument checks and the packing of the
// descriptor list into by-value kernel arguments) on its own, for the HOST sanitizers; the launch is a stub that
// inspects the pack it is handed.  CPU only - it never touches a device:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/micro/ema_host_check.hip -o tools/micro/ema_host_check && tools/micro/ema_host_check
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../care_amd/csrc/ema_pack.h"

static int failures = 0;
static int checks = 0;
#define EXPECT(COND)                                                   \
  do {                                                                 \
    ++checks;                                                          \
    if (!(COND)) { printf("FAILED line %d: %s\n", __LINE__, #COND); ++failures; } \
  } while (0)

// descriptors over fake, never dereferenced addresses: tensor i has sizes[i] elements
static std::vector<care_ema_tensor> make(const std::vector<int64_t>& sizes) {
  std::vector<care_ema_tensor> ts(sizes.size());
  uintptr_t at = 4096;
  for (size_t i = 0; i < sizes.size(); ++i) {
    ts[i].t = (float*)at;
    ts[i].s = (const float*)(at + 4);
    ts[i].n = sizes[i];
    at += 64;
  }
  return ts;
}

struct seen { int launches = 0; int64_t chunks = 0; int tensors = 0; };

// walks a checked list through the stub and checks every pack against the list
static seen walk(const std::vector<care_ema_tensor>& ts) {
  seen s;
  const int rc = care_ema_for_each_pack(ts.data(), (int)ts.size(), [&](const care_ema_pack& pk, int chunks, int li) {
    EXPECT(li == s.launches);
    EXPECT(pk.count >= 1 && pk.count <= CARE_EMA_PACK);
    EXPECT(pk.start[0] == 0 && pk.start[pk.count] == chunks);
    for (int i = 0; i < pk.count; ++i) {
      const care_ema_tensor& want = ts[(size_t)(s.tensors + i)];
      EXPECT(pk.t[i].t == want.t && pk.t[i].s == want.s && pk.t[i].n == want.n);
      EXPECT(pk.start[i + 1] - pk.start[i] == (int32_t)care_ema_chunks(want.n));
      // the kernel's walk: a tensor owns a chunk only if it has elements there, and its last chunk ends at n
      EXPECT((pk.start[i + 1] == pk.start[i]) == (want.n == 0));
      if (want.n > 0) {
        const int64_t last = (int64_t)(pk.start[i + 1] - 1 - pk.start[i]) * CARE_EMA_CHUNK;
        EXPECT(last < want.n && want.n - last <= CARE_EMA_CHUNK);
      }
    }
    for (int i = pk.count; i < CARE_EMA_PACK; ++i) {
      EXPECT(pk.t[i].t == nullptr && pk.t[i].s == nullptr && pk.t[i].n == 0 && pk.start[i + 1] == chunks);
    }
    s.launches += 1; s.chunks += chunks; s.tensors += pk.count;
    return 0;
  });
  EXPECT(rc == 0);
  return s;
}

int main() {
  static_assert(sizeof(care_ema_tensor) == 24, "t, s, n");
  static_assert(sizeof(care_ema_pack) + 3 * sizeof(int32_t) <= 4096, "the pack, the chunk count and both weights fit the argument block");
  // zero tensors: accepted, nothing launched
  EXPECT(care_ema_check(nullptr, 0) == 0);
  EXPECT(walk({}).launches == 0);
  EXPECT(care_ema_chunks(0) == 0 && care_ema_chunks(1) == 1 && care_ema_chunks(1023) == 1 && care_ema_chunks(1024) == 1);
  EXPECT(care_ema_chunks(1025) == 2 && care_ema_chunks(INT64_MAX) == INT64_MAX / 1024 + 1);

  // one tensor, at each size around a chunk
  for (int64_t n : {(int64_t)1, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)52736}) {
    auto ts = make({n});
    EXPECT(care_ema_check(ts.data(), 1) == 0);
    const seen s = walk(ts);
    EXPECT(s.launches == 1 && s.tensors == 1 && s.chunks == (n + 1023) / 1024);
  }
  // one launch: the sizes of the tests; empty tensors at the head, in the middle and at the tail
  {
    auto ts = make({0, 1, 3, 4, 5, 0, 1023, 1024, 1025, 0, 0, 4099, 52736, 0});
    EXPECT(care_ema_check(ts.data(), (int)ts.size()) == 0);
    const seen s = walk(ts);
    EXPECT(s.launches == 1 && s.tensors == 14 && s.chunks == 4 + 1 + 1 + 2 + 5 + 52);
  }
  // a list of empty tensors only: one pack without a chunk (the launcher skips it)
  {
    auto ts = make({0, 0, 0});
    EXPECT(care_ema_check(ts.data(), 3) == 0);
    const seen s = walk(ts);
    EXPECT(s.launches == 1 && s.chunks == 0);
  }
  // more tensors than one launch holds: exactly one pack, one more, and several
  for (int count : {CARE_EMA_PACK, CARE_EMA_PACK + 1, 2 * CARE_EMA_PACK + 2, 3 * CARE_EMA_PACK + 7}) {
    std::vector<int64_t> sizes((size_t)count);
    for (int i = 0; i < count; ++i) sizes[(size_t)i] = 1 + i % 40;
    auto ts = make(sizes);
    EXPECT(care_ema_check(ts.data(), count) == 0);
    const seen s = walk(ts);
    EXPECT(s.launches == (count + CARE_EMA_PACK - 1) / CARE_EMA_PACK && s.tensors == count && s.chunks == count);
  }
  // a failing launch ends the walk and is handed on
  {
    auto ts = make(std::vector<int64_t>(300, 2000));
    int calls = 0;
    EXPECT(care_ema_for_each_pack(ts.data(), 300, [&](const care_ema_pack&, int, int) { return ++calls == 2 ? 719 : 0; }) == 719 && calls == 2);
  }
  // every refused argument
  {
    auto ts = make({8, 8, 8});
    EXPECT(care_ema_check(nullptr, 3) == CARE_EINVAL);
    EXPECT(care_ema_check(ts.data(), -1) == CARE_EINVAL);
    auto bad = ts;
    bad[1].t = nullptr;
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EINVAL);
    bad = ts;
    bad[1].s = nullptr;
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EINVAL);
    bad = ts;
    bad[2].n = -1;
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EINVAL);
    bad = ts;
    bad[2].s = bad[2].t;           // a tensor paired with itself
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EINVAL);
    bad[2].n = 0;                  // ... also an empty one
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EINVAL);
    bad = ts;
    bad[0].t = (float*)(uintptr_t)(4096 + 2);
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EALIGN);
    bad = ts;
    bad[2].s = (const float*)(uintptr_t)(8192 + 1);
    EXPECT(care_ema_check(bad.data(), 3) == CARE_EALIGN);
    bad = ts;
    bad[0].n = INT64_MAX;          // more chunks than a launch can number, and no overflow on the way
    bad[1].n = INT64_MAX;
    EXPECT(care_ema_check(bad.data(), 3) == CARE_ESHAPE);
    bad[0].n = (int64_t)1 << 42;
    bad[1].n = 0; bad[2].n = 0;
    EXPECT(care_ema_check(bad.data(), 3) == CARE_ESHAPE);
    bad[0].n = ((int64_t)0x7fffffff) * CARE_EMA_CHUNK;   // the most one launch takes
    EXPECT(care_ema_check(bad.data(), 3) == 0);
    const seen s = walk(bad);
    EXPECT(s.launches == 1 && s.chunks == 0x7fffffff);
    bad[1].n = 1;                  // one chunk more
    EXPECT(care_ema_check(bad.data(), 3) == CARE_ESHAPE);
    // the limit is per launch: the same two tensors in different packs are taken
    std::vector<int64_t> sizes((size_t)CARE_EMA_PACK + 1, 0);
    sizes[0] = ((int64_t)0x7fffffff) * CARE_EMA_CHUNK;
    sizes[(size_t)CARE_EMA_PACK] = 1;
    auto two = make(sizes);
    EXPECT(care_ema_check(two.data(), (int)two.size()) == 0);
    const seen s2 = walk(two);
    EXPECT(s2.launches == 2 && s2.chunks == (int64_t)0x7fffffff + 1);
  }
  if (failures) { printf("%d of %d check(s) failed\n", failures, checks); return 1; }
  printf("ema_host_check: all %d checks passed\n", checks);
  return 0;
}
