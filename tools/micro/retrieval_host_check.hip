// retrieval_host_check.hip - the host side of csrc/retrieval.hip (csrc/retrieval_plan.h: the argument checks of the four
// entry points and the plan of a care_retrieval_topk call) on its own, for the HOST sanitizers; nothing is launched.
// CPU only - it never touches a device:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/micro/retrieval_host_check.hip -o tools/micro/retrieval_host_check && tools/micro/retrieval_host_check
#include <stdio.h>
#include <stdlib.h>
#include "../../care_amd/csrc/retrieval_plan.h"

static int failures = 0;
#define EXPECT(COND)                                                   \
  do {                                                                 \
    if (!(COND)) { printf("FAILED line %d: %s\n", __LINE__, #COND); ++failures; } \
  } while (0)

// fake, never dereferenced addresses
template <class T> static T* at(uintptr_t a) { return reinterpret_cast<T*>(a); }

struct topk_args {
  const float* q = at<const float>(4096); const float* bank = at<const float>(8192);
  int B = 3, M = 1000, D = 512, topk = 20;
  const int32_t* start = nullptr; const int32_t* end = nullptr; const int32_t* first = nullptr; const int32_t* prev = nullptr;
  const int32_t* orig = nullptr;
  int64_t* ids = at<int64_t>(12288); float* scores = at<float>(16384); int32_t* count = at<int32_t>(20480);
  void* scratch = at<void>(24576); int64_t bytes = (int64_t)1 << 40;
  int check(care_retrieval_plan* pl = nullptr) const {
    care_retrieval_plan own;
    return care_retrieval_topk_check(q, bank, B, M, D, topk, start, end, first, prev, orig, ids, scores, count, scratch, bytes, pl ? pl : &own);
  }
};

// every piece of the scratch inside it, 16-byte aligned, in order and without overlap; the grids cover the shape
static void plan_is_sound(int B, int M, int topk) {
  care_retrieval_plan pl;
  EXPECT(care_retrieval_make_plan(B, M, topk, &pl) == 0);
  EXPECT(pl.bt == pl.qt && (pl.bt == 1 || pl.bt == 2 || pl.bt == 4));
  EXPECT((int64_t)pl.col_blocks * 16 * pl.bt >= M && (int64_t)(pl.col_blocks - 1) * 16 * pl.bt < M);
  EXPECT((int64_t)pl.row_blocks * 16 * pl.qt >= B && (int64_t)(pl.row_blocks - 1) * 16 * pl.qt < B);
  EXPECT((int64_t)pl.groups * 16 >= M && (int64_t)(pl.groups - 1) * 16 < M);
  EXPECT(pl.group_stride % 4 == 0 && pl.group_stride >= pl.groups && (int64_t)pl.col_blocks * pl.bt <= pl.group_stride);
  EXPECT(pl.sort_n >= 16 * topk && pl.sort_n <= 16 * CARE_RETR_MAX_TOPK && (pl.sort_n & (pl.sort_n - 1)) == 0);
  EXPECT(pl.off_gmax == 0 && pl.off_sel >= (int64_t)B * pl.group_stride * 4 && pl.off_nsel >= pl.off_sel + (int64_t)B * topk * 4);
  EXPECT(pl.off_cand >= pl.off_nsel + (int64_t)B * 4 && pl.bytes == pl.off_cand + (int64_t)B * topk * 128);
  EXPECT(pl.off_sel % 16 == 0 && pl.off_nsel % 16 == 0 && pl.off_cand % 16 == 0);
}

int main() {
  for (int B : {1, 2, 15, 16, 17, 32, 33, 37, 64, 65, 2048})
    for (int M : {1, 15, 16, 17, 50, 63, 64, 65, 1000, 130260, CARE_RETR_MAX_M})
      for (int topk : {1, 20, 100, 128}) plan_is_sound(B, M, topk);
  {
    care_retrieval_plan pl;
    EXPECT(care_retrieval_make_plan(16, 1000, 20, &pl) == 0 && pl.bt == 1 && pl.col_blocks == 63 && pl.row_blocks == 1);
    EXPECT(care_retrieval_make_plan(17, 1000, 20, &pl) == 0 && pl.bt == 2 && pl.col_blocks == 32 && pl.row_blocks == 1);
    EXPECT(care_retrieval_make_plan(37, 1000, 100, &pl) == 0 && pl.bt == 4 && pl.col_blocks == 16 && pl.row_blocks == 1 && pl.sort_n == 2048);
    EXPECT(care_retrieval_make_plan(2048, 130260, 20, &pl) == 0 && pl.col_blocks == 2036 && pl.row_blocks == 32 && pl.groups == 8142 &&
           pl.group_stride == 8144 && pl.sort_n == 512);
    for (int bad_b : {0, -1}) EXPECT(care_retrieval_make_plan(bad_b, 1000, 20, &pl) == CARE_ESHAPE);
    for (int bad_m : {0, -7, CARE_RETR_MAX_M + 1, 0x7fffffff}) EXPECT(care_retrieval_make_plan(1, bad_m, 20, &pl) == CARE_ESHAPE);
    for (int bad_k : {0, -1, 129, 1 << 20}) EXPECT(care_retrieval_make_plan(1, 1000, bad_k, &pl) == CARE_ESHAPE);
    // more workgroups than a grid's x dimension numbers
    EXPECT(care_retrieval_make_plan(0x7fffffff, CARE_RETR_MAX_M, 1, &pl) == CARE_ESHAPE);
  }
  // care_retrieval_topk: every refused argument
  {
    topk_args ok;
    care_retrieval_plan pl;
    EXPECT(ok.check(&pl) == 0 && pl.bytes == 64 * 4 * 3 + 240 + 16 + 3 * 20 * 128);
    { topk_args a; a.q = nullptr; EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.bank = nullptr; EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.ids = nullptr; EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.scores = nullptr; EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.count = nullptr; EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.scratch = nullptr; EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.first = at<const int32_t>(64); EXPECT(a.check() == CARE_EINVAL); }      // a `first` without a `prev`
    { topk_args a; a.prev = at<const int32_t>(64); EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.start = at<const int32_t>(64); EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.end = at<const int32_t>(64); EXPECT(a.check() == CARE_EINVAL); }
    { topk_args a; a.first = at<const int32_t>(64); a.prev = at<const int32_t>(128); a.start = at<const int32_t>(196);
      a.end = at<const int32_t>(256); a.orig = at<const int32_t>(260); EXPECT(a.check() == 0); }
    { topk_args a; a.bytes = pl.bytes - 1; EXPECT(a.check() == CARE_EINVAL); a.bytes = pl.bytes; EXPECT(a.check() == 0); }
    for (int D : {0, -16, 8, 24, 500, 1040, 4096}) { topk_args a; a.D = D; EXPECT(a.check() == CARE_ESHAPE); }
    for (int D : {16, 512, 640, 768, 1024}) { topk_args a; a.D = D; EXPECT(a.check() == 0); }
    { topk_args a; a.topk = 0; EXPECT(a.check() == CARE_ESHAPE); a.topk = 129; EXPECT(a.check() == CARE_ESHAPE); a.topk = 128; EXPECT(a.check() == 0); }
    { topk_args a; a.M = 0; EXPECT(a.check() == CARE_ESHAPE); a.M = 1; EXPECT(a.check() == 0); }
    { topk_args a; a.B = -1; EXPECT(a.check() == CARE_ESHAPE); a.B = 0; EXPECT(a.check() == CARE_ESHAPE); }
    { topk_args a; a.q = at<const float>(4100); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.bank = at<const float>(8200); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.scratch = at<void>(24584); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.ids = at<int64_t>(12292); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.scores = at<float>(16386); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.count = at<int32_t>(20481); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.orig = at<const int32_t>(66); EXPECT(a.check() == CARE_EALIGN); }
    { topk_args a; a.start = at<const int32_t>(64); a.end = at<const int32_t>(130); EXPECT(a.check() == CARE_EALIGN); }
  }
  // the other three
  {
    const float* x = at<const float>(4096);
    float* y = at<float>(8192);
    const int64_t* ids = at<const int64_t>(12288);
    EXPECT(care_l2_normalize_rows_check(x, y, 1000, 512) == 0 && care_l2_normalize_rows_check(x, y, 1, 16) == 0);
    EXPECT(care_l2_normalize_rows_check(nullptr, y, 10, 512) == CARE_EINVAL && care_l2_normalize_rows_check(x, nullptr, 10, 512) == CARE_EINVAL);
    EXPECT(care_l2_normalize_rows_check(x, y, 0, 512) == CARE_ESHAPE && care_l2_normalize_rows_check(x, y, 10, 520) == CARE_ESHAPE);
    EXPECT(care_l2_normalize_rows_check(x, y, 10, 1040) == CARE_ESHAPE && care_l2_normalize_rows_check(x, y, 0x7fffffff, 512) == CARE_ESHAPE);
    EXPECT(care_l2_normalize_rows_check(at<const float>(4104), y, 10, 512) == CARE_EALIGN);
    EXPECT(care_retrieval_query_check(x, y, 3, 28, 512) == 0 && care_retrieval_query_check(x, y, 1, 1, 1024) == 0);
    EXPECT(care_retrieval_query_check(nullptr, y, 3, 28, 512) == CARE_EINVAL && care_retrieval_query_check(x, nullptr, 3, 28, 512) == CARE_EINVAL);
    EXPECT(care_retrieval_query_check(x, y, 0, 28, 512) == CARE_ESHAPE && care_retrieval_query_check(x, y, 3, 0, 512) == CARE_ESHAPE);
    EXPECT(care_retrieval_query_check(x, y, 3, 28, 100) == CARE_ESHAPE && care_retrieval_query_check(x, at<float>(8196), 3, 28, 512) == CARE_EALIGN);
    EXPECT(care_retrieval_gather_check(x, 10, 768, ids, 4, y) == 0);
    EXPECT(care_retrieval_gather_check(nullptr, 10, 768, ids, 4, y) == CARE_EINVAL && care_retrieval_gather_check(x, 10, 768, nullptr, 4, y) == CARE_EINVAL);
    EXPECT(care_retrieval_gather_check(x, 10, 768, ids, 4, nullptr) == CARE_EINVAL);
    EXPECT(care_retrieval_gather_check(x, 0, 768, ids, 4, y) == CARE_ESHAPE && care_retrieval_gather_check(x, 10, 776, ids, 4, y) == CARE_ESHAPE);
    EXPECT(care_retrieval_gather_check(x, 10, 768, ids, 0, y) == CARE_ESHAPE);
    EXPECT(care_retrieval_gather_check(x, 10, 768, at<const int64_t>(12292), 4, y) == CARE_EALIGN);
    EXPECT(care_retrieval_gather_check(x, 10, 768, ids, 4, at<float>(8200)) == CARE_EALIGN);
  }
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("retrieval_host_check: all checks passed\n");
  return 0;
}
