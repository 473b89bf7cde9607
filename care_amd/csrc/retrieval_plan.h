// retrieval_plan.h - the HOST side of retrieval.hip: the argument checks of the four entry points and the plan of a
// care_retrieval_topk call (which scan form, the grids, where each piece of the scratch lies).  Plain C++ with no HIP in
// it, so tools/micro/retrieval_host_check.hip runs exactly this code under the host sanitizers without any launch.
#pragma once
#include <stdint.h>
#include "../../include/care_hip.h"

constexpr int CARE_RETR_GROUP = 16;      // columns of a group: one MFMA tile of bank rows
constexpr int CARE_RETR_MAX_TOPK = 128;
constexpr int CARE_RETR_MAX_D = 1024;
constexpr int CARE_RETR_MAX_M = 0x7fffffff - 63;

struct care_retrieval_plan {
  int bt, qt;              // the scan form: a wave owns bt groups of 16 columns x qt tiles of 16 rows
  int col_blocks, row_blocks;
  int groups;              // ceil(M / 16)
  int group_stride;        // floats between two rows of the group maxima: 4 ceil(M / 64)
  int sort_n;              // candidates the ranking sorts: the power of two >= 16 topk
  int64_t off_gmax, off_sel, off_nsel, off_cand, bytes;   // the scratch: fp32 [B, group_stride], int32 [B, topk], int32 [B], uint64 [B, topk, 16]
};

static inline int64_t care_retr_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

static inline bool care_retr_dim_ok(int D) { return D >= 16 && D <= CARE_RETR_MAX_D && D % 16 == 0; }

// the shapes of a scan; CARE_ESHAPE when unsupported
static inline int care_retrieval_make_plan(int B, int M, int topk, care_retrieval_plan* pl) {
  if (B < 1 || M < 1 || M > CARE_RETR_MAX_M || topk < 1 || topk > CARE_RETR_MAX_TOPK) return CARE_ESHAPE;
  // up to 16 rows the scan is bound by the bank's bytes: a wave per group, so that every SIMD has several in flight;
  // beyond 32 rows by the matrix pipe: 4 x 4 tiles a wave, 16 independent accumulators per operand pair
  pl->bt = pl->qt = B <= 16 ? 1 : B <= 32 ? 2 : 4;
  pl->col_blocks = (int)(((int64_t)M + 16 * pl->bt - 1) / (16 * pl->bt));
  pl->row_blocks = (int)(((int64_t)B + 16 * pl->qt - 1) / (16 * pl->qt));
  if ((int64_t)pl->col_blocks * pl->row_blocks > 0x7fffffff || (int64_t)B * topk > 0x7fffffff) return CARE_ESHAPE;
  pl->groups = (int)(((int64_t)M + 15) / 16);
  pl->group_stride = (int)(((int64_t)M + 63) / 64) * 4;
  pl->sort_n = 16;
  while (pl->sort_n < 16 * topk) pl->sort_n *= 2;
  pl->off_gmax = 0;
  pl->off_sel = care_retr_up16((int64_t)B * pl->group_stride * 4);
  pl->off_nsel = pl->off_sel + care_retr_up16((int64_t)B * topk * 4);
  pl->off_cand = pl->off_nsel + care_retr_up16((int64_t)B * 4);
  pl->bytes = pl->off_cand + (int64_t)B * topk * 16 * 8;
  return 0;
}

static inline int care_l2_normalize_rows_check(const float* x, float* y, int M, int D) {
  if (!x || !y) return CARE_EINVAL;
  if (M < 1 || M > CARE_RETR_MAX_M || !care_retr_dim_ok(D)) return CARE_ESHAPE;
  if ((((uintptr_t)x) | ((uintptr_t)y)) & 15u) return CARE_EALIGN;
  return 0;
}

static inline int care_retrieval_query_check(const float* frames, float* q, int B, int n, int D) {
  if (!frames || !q) return CARE_EINVAL;
  if (B < 1 || n < 1 || !care_retr_dim_ok(D)) return CARE_ESHAPE;
  if ((((uintptr_t)frames) | ((uintptr_t)q)) & 15u) return CARE_EALIGN;
  return 0;
}

static inline int care_retrieval_topk_check(const float* q, const float* bank, int B, int M, int D, int topk, const int32_t* start,
                                            const int32_t* end, const int32_t* first, const int32_t* prev, const int32_t* orig,
                                            const int64_t* ids, const float* scores, const int32_t* count, const void* scratch,
                                            int64_t scratch_bytes, care_retrieval_plan* pl) {
  if (!q || !bank || !ids || !scores || !count || !scratch) return CARE_EINVAL;
  if ((start == nullptr) != (end == nullptr) || (first == nullptr) != (prev == nullptr)) return CARE_EINVAL;
  if (!care_retr_dim_ok(D)) return CARE_ESHAPE;
  const int rc = care_retrieval_make_plan(B, M, topk, pl);
  if (rc) return rc;
  if (scratch_bytes < pl->bytes) return CARE_EINVAL;
  if ((((uintptr_t)q) | ((uintptr_t)bank) | ((uintptr_t)scratch)) & 15u) return CARE_EALIGN;
  if ((((uintptr_t)start) | ((uintptr_t)end) | ((uintptr_t)first) | ((uintptr_t)prev) | ((uintptr_t)orig) | ((uintptr_t)scores) |
       ((uintptr_t)count)) & 3u)
    return CARE_EALIGN;
  if (((uintptr_t)ids) & 7u) return CARE_EALIGN;
  return 0;
}

static inline int care_retrieval_gather_check(const float* table, int rows, int De, const int64_t* ids, int n, const float* out) {
  if (!table || !ids || !out) return CARE_EINVAL;
  if (rows < 1 || n < 1 || !care_retr_dim_ok(De)) return CARE_ESHAPE;
  if ((((uintptr_t)table) | ((uintptr_t)out)) & 15u) return CARE_EALIGN;
  if (((uintptr_t)ids) & 7u) return CARE_EALIGN;
  return 0;
}
