// sweep_host_check.hip - the host side of csrc/sweep.h (the argument checks of care_grad_sqnorm / care_adam_step and of
// care_ema_step, and the packing of a descriptor list into by-value kernel arguments) on its own, for the HOST sanitizers;
// the launch is a stub that inspects the pack it is handed.  One harness, run for both descriptors.  CPU only - it never
// touches a device:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/micro/sweep_host_check.hip -o tools/micro/sweep_host_check && tools/micro/sweep_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../care_amd/csrc/sweep.h"

static int failures = 0;
static int checks = 0;
#define EXPECT(COND)                                                   \
  do {                                                                 \
    ++checks;                                                          \
    if (!(COND)) { printf("FAILED line %d: %s\n", __LINE__, #COND); ++failures; } \
  } while (0)

constexpr int64_t MOST = ((int64_t)0x7fffffff) * CARE_SWEEP_CHUNK;  // the most elements one launch takes

// descriptors over fake, never dereferenced addresses: tensor i has sizes[i] elements
static std::vector<care_opt_tensor> make_opt(const std::vector<int64_t>& sizes) {
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

static std::vector<care_ema_tensor> make_ema(const std::vector<int64_t>& sizes) {
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

// walks a checked list through the stub and checks every pack against the list (both descriptors are without padding:
// equal bytes are equal fields)
template <int N, class T>
static seen walk(const std::vector<T>& ts) {
  seen s;
  const T none = {};
  const int rc = care_sweep_for_each_pack<N>(ts.data(), (int)ts.size(), [&](const care_sweep_pack<T, N>& pk, int chunks, int li) {
    EXPECT(li == s.launches);
    EXPECT(pk.count >= 1 && pk.count <= N);
    EXPECT(pk.start[0] == 0 && pk.start[pk.count] == chunks);
    for (int i = 0; i < pk.count; ++i) {
      const T& want = ts[(size_t)(s.tensors + i)];
      EXPECT(memcmp(&pk.t[i], &want, sizeof(T)) == 0);
      EXPECT(pk.start[i + 1] - pk.start[i] == (int32_t)care_sweep_chunks(want.n));
      // the kernel's walk: a tensor owns a chunk only if it has elements there, and its last chunk ends at n
      EXPECT((pk.start[i + 1] == pk.start[i]) == (want.n == 0));
      if (want.n > 0) {
        const int64_t last = (int64_t)(pk.start[i + 1] - 1 - pk.start[i]) * CARE_SWEEP_CHUNK;
        EXPECT(last < want.n && want.n - last <= CARE_SWEEP_CHUNK);
      }
    }
    for (int i = pk.count; i < N; ++i) EXPECT(memcmp(&pk.t[i], &none, sizeof(T)) == 0 && pk.start[i + 1] == chunks);
    s.launches += 1; s.chunks += chunks; s.tensors += pk.count;
    return 0;
  });
  EXPECT(rc == 0);
  return s;
}

// everything the two lists share.  pointers: the descriptor begins with that many pointers, every one of them checked
template <int N, class T, class Make, class Check>
static void suite(Make make, Check check, int pointers) {
  static_assert(sizeof(care_sweep_pack<T, N>) + 9 * sizeof(int32_t) <= 4096, "the pack and the kernel's scalars fit the argument block");
  // zero tensors: accepted, nothing launched
  EXPECT(check(nullptr, 0) == 0);
  EXPECT((walk<N, T>({}).launches == 0));
  // one tensor, at each size around a chunk
  for (int64_t n : {(int64_t)1, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)52736}) {
    auto ts = make({n});
    EXPECT(check(ts.data(), 1) == 0);
    const seen s = walk<N>(ts);
    EXPECT(s.launches == 1 && s.tensors == 1 && s.chunks == (n + 1023) / 1024);
  }
  // one launch: the sizes of the tests; empty tensors at the head, in the middle and at the tail
  {
    auto ts = make({1, 3, 4, 5, 0, 500, 912, 1023, 1024, 1025, 65537, 300001});
    EXPECT(check(ts.data(), (int)ts.size()) == 0);
    seen s = walk<N>(ts);
    EXPECT(s.launches == 1 && s.tensors == 12 && s.chunks == 4 + 0 + 4 + 2 + 65 + 293);
    ts = make({0, 1, 3, 4, 5, 0, 1023, 1024, 1025, 0, 0, 4099, 52736, 0});
    EXPECT(check(ts.data(), (int)ts.size()) == 0);
    s = walk<N>(ts);
    EXPECT(s.launches == 1 && s.tensors == 14 && s.chunks == 4 + 1 + 1 + 2 + 5 + 52);
  }
  // a list of empty tensors only: one pack without a chunk (the launchers skip it)
  {
    auto ts = make({0, 0, 0});
    EXPECT(check(ts.data(), 3) == 0);
    const seen s = walk<N>(ts);
    EXPECT(s.launches == 1 && s.chunks == 0);
  }
  // more tensors than one launch holds: exactly one pack, one more, and several
  for (int count : {N, N + 1, 2 * N + 2, 3 * N + 7}) {
    std::vector<int64_t> sizes((size_t)count);
    for (int i = 0; i < count; ++i) sizes[(size_t)i] = 1 + i % 40;
    auto ts = make(sizes);
    EXPECT(check(ts.data(), count) == 0);
    const seen s = walk<N>(ts);
    EXPECT(s.launches == (count + N - 1) / N && s.tensors == count && s.chunks == count);
  }
  // a failing launch ends the walk and is handed on
  {
    auto ts = make(std::vector<int64_t>((size_t)(2 * N + 22), 2000));
    int calls = 0;
    EXPECT(care_sweep_for_each_pack<N>(ts.data(), (int)ts.size(), [&](const care_sweep_pack<T, N>&, int, int) { return ++calls == 2 ? 719 : 0; }) == 719 &&
           calls == 2);
  }
  // every refused argument
  const auto ts = make({8, 8, 8});
  EXPECT(check(nullptr, 3) == CARE_EINVAL);
  EXPECT(check(ts.data(), -1) == CARE_EINVAL);
  for (int field = 0; field < pointers; ++field) {
    for (int i = 0; i < 3; ++i) {
      auto bad = ts;
      uintptr_t at = 0;
      memcpy((char*)&bad[(size_t)i] + (size_t)field * sizeof at, &at, sizeof at);
      EXPECT(check(bad.data(), 3) == CARE_EINVAL);
      for (uintptr_t off : {1, 2, 3}) {
        at = 8192 + off;
        memcpy((char*)&bad[(size_t)i] + (size_t)field * sizeof at, &at, sizeof at);
        EXPECT(check(bad.data(), 3) == CARE_EALIGN);
      }
    }
  }
  auto bad = ts;
  bad[2].n = -1;
  EXPECT(check(bad.data(), 3) == CARE_EINVAL);
  bad = ts;
  bad[0].n = INT64_MAX;          // too much for a launch or for the sum of the sizes, and no overflow on the way
  bad[1].n = INT64_MAX;
  EXPECT(check(bad.data(), 3) == CARE_ESHAPE);
  bad[1].n = 0; bad[2].n = 0;    // ... nor in the chunk count of ONE such tensor
  EXPECT(check(bad.data(), 3) == CARE_ESHAPE);
  bad[0].n = (int64_t)1 << 42;   // more chunks than a launch can number
  EXPECT(check(bad.data(), 3) == CARE_ESHAPE);
  bad[0].n = MOST;
  EXPECT(check(bad.data(), 3) == 0);
  const seen s = walk<N>(bad);
  EXPECT(s.launches == 1 && s.chunks == 0x7fffffff);
  bad[1].n = 1;                  // one chunk more
  EXPECT(check(bad.data(), 3) == CARE_ESHAPE);
  // the limit is per launch: the same two tensors in different packs are taken
  std::vector<int64_t> sizes((size_t)N + 1, 0);
  sizes[0] = MOST;
  sizes[(size_t)N] = 1;
  auto two = make(sizes);
  EXPECT(check(two.data(), (int)two.size()) == 0);
  const seen s2 = walk<N>(two);
  EXPECT(s2.launches == 2 && s2.chunks == (int64_t)0x7fffffff + 1);
}

int main() {
  EXPECT(care_sweep_chunks(0) == 0 && care_sweep_chunks(1) == 1 && care_sweep_chunks(1023) == 1 && care_sweep_chunks(1024) == 1);
  EXPECT(care_sweep_chunks(1025) == 2 && care_sweep_chunks(INT64_MAX) == INT64_MAX / 1024 + 1);
  EXPECT(care_sweep_grid(0) == 1 && care_sweep_grid(1) == 1 && care_sweep_grid(2) == 2 && care_sweep_grid(2048) == 2048);
  EXPECT(care_sweep_grid(care_sweep_chunks(18218884)) == 2048 && care_sweep_grid(care_sweep_chunks((int64_t)1 << 40)) == 2048);

  static_assert(sizeof(care_opt_tensor) == 48 && sizeof(care_ema_tensor) == 24, "four pointers, n, two floats; t, s, n");
  suite<CARE_OPT_PACK, care_opt_tensor>(make_opt, [](const care_opt_tensor* ts, int n) { return care_opt_check(ts, n, nullptr); }, 4);
  suite<CARE_EMA_PACK, care_ema_tensor>(make_ema, care_ema_check, 2);

  // the optimiser's list also reports the sum of its sizes, and refuses one that does not fit an int64
  {
    int64_t total = -1;
    EXPECT(care_opt_check(nullptr, 0, &total) == 0 && total == 0);
    auto ts = make_opt({1, 3, 4, 5, 0, 500, 912, 1023, 1024, 1025, 65537, 300001});
    EXPECT(care_opt_check(ts.data(), (int)ts.size(), &total) == 0 && total == 1 + 3 + 4 + 5 + 500 + 912 + 1023 + 1024 + 1025 + 65537 + 300001);
    ts = make_opt({INT64_MAX, 8, 8});
    EXPECT(care_opt_check(ts.data(), 3, &total) == CARE_ESHAPE);
    ts = make_opt({INT64_MAX});    // the sum fits; the chunk count must not overflow on the way to the refusal
    EXPECT(care_opt_check(ts.data(), 1, &total) == CARE_ESHAPE);
    // the rules of a tensor come in index order, before the limit of a launch
    ts = make_opt({(int64_t)1 << 42, 8, -1});
    EXPECT(care_opt_check(ts.data(), 3, &total) == CARE_EINVAL);
  }
  // the teacher's list refuses a tensor paired with itself, also an empty one
  {
    auto ts = make_ema({8, 8, 8});
    ts[2].s = ts[2].t;
    EXPECT(care_ema_check(ts.data(), 3) == CARE_EINVAL);
    ts[2].n = 0;
    EXPECT(care_ema_check(ts.data(), 3) == CARE_EINVAL);
  }
  if (failures) { printf("%d of %d check(s) failed\n", failures, checks); return 1; }
  printf("sweep_host_check: all %d checks passed\n", checks);
  return 0;
}
