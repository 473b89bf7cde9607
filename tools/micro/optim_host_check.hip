// optim_host_check.hip - the host launcher of csrc/optim.hip (csrc/optim_pack.h: argument checks and the packing of the
// descriptor list into by-value kernel arguments) on its own, for the HOST sanitizers; the launch is a stub that
// inspects the pack it is handed.  CPU only - it never touches a device:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/micro/optim_host_check.hip -o tools/micro/optim_host_check && tools/micro/optim_host_check
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../care_amd/csrc/optim_pack.h"

static int failures = 0;
#define EXPECT(COND)                                                   \
  do {                                                                 \
    if (!(COND)) { printf("FAILED line %d: %s\n", __LINE__, #COND); ++failures; } \
  } while (0)

// descriptors over fake, never dereferenced addresses: tensor i has sizes[i] elements
static std::vector<care_opt_tensor> make(const std::vector<int64_t>& sizes) {
  std::vector<care_opt_tensor> ts(sizes.size());
  uintptr_t at = 4096;
  for (size_t i = 0; i < sizes.size(); ++i) {
    care_opt_tensor& d = ts[i];
    d.p = (float*)at; d.g = (const float*)(at + 4); d.m = (float*)(at + 8); d.v = (float*)(at + 12);
    d.n = sizes[i]; d.step_size = 1e-3f * (float)(i + 1); d.weight_decay = (i & 1) ? 1e-3f : 0.f;
    at += 64;
  }
  return ts;
}

static void set_pointer(care_opt_tensor& d, int field, uintptr_t at) {
  if (field == 0) d.p = (float*)at;
  else if (field == 1) d.g = (const float*)at;
  else if (field == 2) d.m = (float*)at;
  else d.v = (float*)at;
}

struct seen { int launches = 0; int64_t chunks = 0; int tensors = 0; };

// walks a checked list through the stub and checks every pack against the list
static seen walk(const std::vector<care_opt_tensor>& ts) {
  seen s;
  const int rc = care_opt_for_each_pack(ts.data(), (int)ts.size(), [&](const care_opt_pack& pk, int chunks, int li) {
    EXPECT(li == s.launches);
    EXPECT(pk.count >= 1 && pk.count <= CARE_OPT_PACK);
    EXPECT(pk.start[0] == 0 && pk.start[pk.count] == chunks);
    for (int i = 0; i < pk.count; ++i) {
      const care_opt_tensor& want = ts[(size_t)(s.tensors + i)];
      EXPECT(pk.t[i].p == want.p && pk.t[i].g == want.g && pk.t[i].m == want.m && pk.t[i].v == want.v && pk.t[i].n == want.n);
      EXPECT(pk.t[i].step_size == want.step_size && pk.t[i].weight_decay == want.weight_decay);
      EXPECT(pk.start[i + 1] - pk.start[i] == (int32_t)care_opt_chunks(want.n));
    }
    for (int i = pk.count; i < CARE_OPT_PACK; ++i) {
      EXPECT(pk.t[i].p == nullptr && pk.t[i].n == 0 && pk.start[i + 1] == chunks);
    }
    s.launches += 1; s.chunks += chunks; s.tensors += pk.count;
    return 0;
  });
  EXPECT(rc == 0);
  return s;
}

int main() {
  int64_t total = -1;
  // zero tensors: accepted, nothing launched
  EXPECT(care_opt_check(nullptr, 0, &total) == 0 && total == 0);
  EXPECT(walk({}).launches == 0);
  EXPECT(care_opt_partials(0) == 1 && care_opt_partials(1) == 1 && care_opt_partials(1024) == 1 && care_opt_partials(1025) == 2);
  EXPECT(care_opt_partials(18218884) == 2048 && care_opt_partials((int64_t)1 << 40) == 2048);

  // one launch: the sizes of the tests, an empty tensor among them
  {
    auto ts = make({1, 3, 4, 5, 0, 500, 912, 1023, 1024, 1025, 65537, 300001});
    EXPECT(care_opt_check(ts.data(), (int)ts.size(), &total) == 0 && total == 1 + 3 + 4 + 5 + 500 + 912 + 1023 + 1024 + 1025 + 65537 + 300001);
    const seen s = walk(ts);
    EXPECT(s.launches == 1 && s.tensors == 12 && s.chunks == 4 + 0 + 4 + 2 + 65 + 293);
  }
  // more tensors than one launch holds: exactly one pack, one more, and several
  for (int count : {CARE_OPT_PACK, CARE_OPT_PACK + 1, 80, 3 * CARE_OPT_PACK + 7}) {
    auto ts = make(std::vector<int64_t>((size_t)count, 5));
    EXPECT(care_opt_check(ts.data(), count, &total) == 0 && total == 5 * (int64_t)count);
    const seen s = walk(ts);
    EXPECT(s.launches == (count + CARE_OPT_PACK - 1) / CARE_OPT_PACK && s.tensors == count && s.chunks == count);
  }
  // a failing launch ends the walk and is handed on
  {
    auto ts = make(std::vector<int64_t>(150, 2000));
    int calls = 0;
    EXPECT(care_opt_for_each_pack(ts.data(), 150, [&](const care_opt_pack&, int, int) { return ++calls == 2 ? 719 : 0; }) == 719 && calls == 2);
  }
  // every refused argument
  {
    auto ts = make({8, 8, 8});
    EXPECT(care_opt_check(nullptr, 3, &total) == CARE_EINVAL);
    EXPECT(care_opt_check(ts.data(), -1, &total) == CARE_EINVAL);
    for (int field = 0; field < 4; ++field) {
      auto bad = ts;
      set_pointer(bad[1], field, 0);
      EXPECT(care_opt_check(bad.data(), 3, &total) == CARE_EINVAL);
      bad = ts;
      set_pointer(bad[2], field, 4096 + 2);
      EXPECT(care_opt_check(bad.data(), 3, &total) == CARE_EALIGN);
    }
    auto bad = ts;
    bad[0].n = -1;
    EXPECT(care_opt_check(bad.data(), 3, &total) == CARE_EINVAL);
    bad[0].n = INT64_MAX;          // the sum of the sizes would overflow
    EXPECT(care_opt_check(bad.data(), 3, &total) == CARE_ESHAPE);
    bad[0].n = (int64_t)1 << 42;   // more chunks than a launch can number
    bad[1].n = 0; bad[2].n = 0;
    EXPECT(care_opt_check(bad.data(), 3, &total) == CARE_ESHAPE);
    bad[0].n = ((int64_t)0x7fffffff) * CARE_OPT_CHUNK;   // the most one launch takes
    EXPECT(care_opt_check(bad.data(), 3, &total) == 0);
    const seen s = walk(bad);
    EXPECT(s.launches == 1 && s.chunks == 0x7fffffff);
  }
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("optim_host_check: all checks passed\n");
  return 0;
}
