// gemm_stream.h - the streamed-W scheme under gemm_as.hip, gemm_vocab.hip, gemm_store32.hip and beam_sparse.hip.
//
// Every GEMM of the decoder has K = d_model = 512 and a tall or huge-N shape, so the kernels keep A still and stream W:
//   * resident A: a wave loads the MFMA A-fragments of its rows for the whole K ONCE, straight from global memory into
//     registers (all loads in flight at once), and keeps them for every column tile of its work item;
//   * a ring of W tiles: W goes through GS_RING LDS slots filled by LDS-DMA (global_load_lds, 16 B per lane, one 1-KiB W
//     row per wave instruction) with GS_AHEAD tiles in flight - the DMA latency (~2 us under load) is several times the
//     MFMAs a wave spends on a tile, so one tile of prefetch leaves the kernel latency-bound (measured: 18 % MFMA
//     occupancy).  beam_sparse.hip holds ONE tile image and no ring;
//   * the image: the DMA writes LDS lane-linearly, so the bank-conflict swizzle (16-byte chunk ^= row & 15) is applied
//     to the per-lane SOURCE address and undone by the ds_read_b128 of the B fragment (conflict-free for every 16-lane
//     read group).  Both halves of that layout are below, next to each other; which source row feeds LDS row n, and how
//     many rows a wave copies, is the kernel's own;
//   * counted waits: s_waitcnt vmcnt(N) with N = the exact number of YOUNGER vector-memory operations (output stores
//     included; care_wait_vm in care_common.h) and a raw s_barrier, so neither the DMAs in flight nor the previous
//     tiles' stores are drained.
// The k-step loops (fragment prefetch, MFMAs, the statistics / epilogue pieces woven between them) are NOT here: that
// is where the kernels differ, and hipcc's register allocation is sensitive to it.
#pragma once
#include "care_common.h"

constexpr int GS_RING = 4;              // LDS ring slots
constexpr int GS_AHEAD = 3;             // tiles in flight
constexpr int GS_ROW = 1024;            // bytes of a W row in LDS: K = 512 16-bit values, 64 chunks of 16 bytes
constexpr int GS_N32 = 32;              // the 32-row image of the 32x32x16 MFMA kernels: columns per tile ...
constexpr int GS_TILE32 = GS_N32 * GS_ROW;  // ... and its bytes
constexpr int GS_ROWS256 = 256;         // rows of a panel of those kernels (8 waves x 32)

// ---- 1. the tile image.  LDS row n holds one W row; the 16-byte source chunk c of it sits at chunk slot c ^ (n & 15).
// Staging: lane = chunk slot, so the lane's source byte offset inside the W row is ...
// (ROWS16: the 16-row tiles of gemm_as.hip, n < 16 - a mask hipcc cannot see to be idle there, so it is left out)
template <bool ROWS16 = false>
__device__ __forceinline__ int gs_src_chunk(int lane, int n) { return (lane ^ (ROWS16 ? n : n & 15)) << 4; }
// ... and one DMA instruction copies the row (g = the lane's source address, lds_row = the row's LDS address).
__device__ __forceinline__ void gs_dma_row(const unsigned char* g, unsigned char* lds_row) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_row, 16, 0, 0);
}
// Reading, 32-row image (v_mfma_f32_32x32x16, lane = (r = lane & 31, h = lane >> 5)): the B fragment of k-step ks is
// chunk 2 ks + h of row r, i.e. slot (2 ks + h) ^ (r & 15): an XOR of the low four chunk bits and 256 bytes per 8 k-steps.
// (the row's own offset r * GS_ROW is the caller's to add: hoisted there, hipcc keeps the kernels' register counts)
__device__ __forceinline__ int gs_frag32(int r, int h, int ks) {
  return ((((2 * ks + h) ^ (r & 15)) & 15) << 4) + ((2 * ks) >> 4) * 256;
}
// With the operands swapped (D = (X W^T)^T) accumulator register i of that lane is LDS row (= tile column) ...
__device__ __forceinline__ int gs_col32(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
// (the 16-row image of gemm_as.hip reads chunk (4 ks + fg) ^ fr of row fr: four distinct offsets per lane, kept there)

// ---- 2. the resident A fragments of a wave's 32 rows (32-row kernels): fragment ks = X[row][16 ks + 8 h + (0..7)];
// rows past M repeat row M - 1
__device__ __forceinline__ void gs_load_a32(bf16x8 (&a)[32], const bf16_t* A, int64_t lda, int row, int M, int h) {
  const bf16_t* arow = A + (int64_t)min(row, M - 1) * lda + h * 8;
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) a[ks] = *reinterpret_cast<const bf16x8*>(arow + ks * 16);
}

// ---- 3. candidate staging (the COLLECT modes: every logit >= its row's threshold goes to the row's candidate list).
// The candidates of a work item are staged in LDS - [0] = count, from byte 8 (value, row-in-panel << 24 | column)
// pairs - and flushed to the global lists once per item.  A global atomic with return inside the tile loop is a full
// memory round trip that also drains the W tiles in flight, and about every second tile of a wave holds a candidate
// (417 us per launch against 257 us for the statistics pass); LDS atomics do not touch vmcnt (asm: through C++ hipcc
// would put a vmcnt(0) in front of them, possible alias with the LDS-DMA).
struct gs_cand_lists {
  int32_t* cnt; float* cval; int32_t* cidx;  // per row: count, values [cap], columns [cap]
  int cap;
};
__device__ __forceinline__ void gs_cand_append(const gs_cand_lists& L, int row, float v, int c) {
  const int pos = atomicAdd(&L.cnt[row], 1);
  if (pos < L.cap) {
    L.cval[(int64_t)row * L.cap + pos] = v;
    L.cidx[(int64_t)row * L.cap + pos] = c;
  }
}
constexpr int gs_cand_lcap(int stage_bytes) { return (stage_bytes - 8) / 8; }
// one thread, before the item's first tile (ordered before the first push by that tile's barrier)
__device__ __forceinline__ void gs_cand_reset(unsigned lbase) {
  const int zero = 0;
  asm volatile("ds_write_b32 %0, %1" ::"v"(lbase), "v"(zero) : "memory");
}
// row0 = the panel's first row, rloc = the row inside the panel (< 256); once the staging area is full: the global list
__device__ __forceinline__ void gs_cand_push(const gs_cand_lists L, unsigned lbase, int lcap, int row0, int rloc, float v, int c) {
  int pos;
  const int one = 1;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(pos) : "v"(lbase), "v"(one) : "memory");
  if (pos < lcap) {
    const unsigned a = lbase + 8 + (unsigned)pos * 8;
    const int packed = (rloc << 24) | c;
    asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" ::"v"(a), "v"(v), "v"(packed) : "memory");
  } else {
    gs_cand_append(L, row0 + rloc, v, c);
  }
}
// after the item's last tile, the whole workgroup (`threads` of it); row0 = the panel's first row
__device__ __forceinline__ void gs_cand_flush(const gs_cand_lists L, unsigned lbase, int lcap, int row0, int tid, int threads) {
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  care_wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  int n;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(n) : "v"(lbase) : "memory");
  n = min(n, lcap);
  for (int e = tid; e < n; e += threads) {
    i32x2 pr;
    const unsigned a = lbase + 8 + (unsigned)e * 8;
    asm volatile("ds_read2_b32 %0, %1 offset1:1\n\ts_waitcnt lgkmcnt(0)" : "=v"(pr) : "v"(a) : "memory");
    gs_cand_append(L, (int)((unsigned)pr[1] >> 24) + row0, __builtin_bit_cast(float, pr[0]), pr[1] & 0xffffff);
  }
}

// ---- 4. partial statistics (max, argmax, sum-exp) of a row over a column range.  The running sum is kept against a
// LAZY reference rref (set from the first tile, moved when the maximum has got more than 20 ahead of it).
// Finite sentinel, not -inf: an update with a masked (-inf) logit then gives exp(-inf) = 0, not NaN.
constexpr float GS_STAT_MIN = -1e30f;
constexpr int GS_STAT_NOIDX = 0x7fffffff;
// the sum relative to the true maximum (rows that saw no logit: rm = rref = -1e30, rs = 0)
__device__ __forceinline__ float gs_stat_close(float rm, float rs, float rref) {
  float s = rs > 0.f ? rs * __expf(rref - rm) : 0.f;
  if (!(s < 3.0e38f)) s = 1.0f;  // the sum overflowed (a > 88 jump inside one tile): it is its largest term
  return s;
}
// merge with the partial of lane ^ o; the lower index wins among equal maxima
__device__ __forceinline__ void gs_stat_merge(float& m, float& s, int& id, int o) {
  const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
  const int oi = __shfl_xor(id, o, 64);
  const float mn = fmaxf(m, om);
  s = s * __expf(m - mn) + os * __expf(om - mn);
  if (om > m || (om == m && oi < id)) id = oi;
  m = mn;
}
// the record of a range that holds no column
__device__ __forceinline__ void gs_stat_empty(float* pmax, int32_t* pidx, float* psum, int64_t o) {
  pmax[o] = -INFINITY; pidx[o] = GS_STAT_NOIDX; psum[o] = 0.f;
}

// ---- 5. destination and bias of the store kernels.  Two destinations like care_gemm_bf16 (columns < n_split -> C0,
// the rest -> C1; each fp32 or 16-bit, own leading dimension); a tile never straddles n_split, so the choice is
// wave-uniform.  p: the kernel's argument struct.
struct gs_dest {
  unsigned char* C; int64_t ld;
  bool isb;    // 16-bit output
  int cshift;  // column of the destination's first column
};
// (a macro, expanded in the kernel: through a function hipcc orders the scalar selects differently)
#define GS_DEST_OF(p, col, slab_bytes)                                                                            \
  gs_dest{reinterpret_cast<unsigned char*>((col) >= (p).n_split ? (p).C1 : (p).C0) + (slab_bytes),                \
          (col) >= (p).n_split ? (p).ldc1 : (p).ldc0, ((col) >= (p).n_split ? (p).c1_bf16 : (p).c0_bf16) != 0,     \
          (col) >= (p).n_split ? (p).n_split : 0}
// The bias slice of a work item's column range is staged in LDS once (nb columns from col0, zero-padded to a multiple
// of 4), behind the prologue DMAs and the A loads: one combined latency ...
__device__ __forceinline__ void gs_bias_stage(float* sb, const float* bias, int col0, int nb, int tid, int threads) {
  for (int i = tid; i < ((nb + 3) & ~3); i += threads) sb[i] = i < nb ? bias[col0 + i] : 0.f;
}
// ... and read back four columns at a time by an asm ds_read (hipcc would put a vmcnt(0) drain in front of a C++ LDS
// read here because the in-flight LDS-DMA might alias it)
__device__ __forceinline__ void gs_bias_read(float4& bv, unsigned lds_addr) {
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(bv) : "v"(lds_addr) : "memory");
}
__device__ __forceinline__ unsigned gs_lds_addr(const unsigned char* smem) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
}

// ---- 6. host side.  The launchers of the 256-row kernels (gemm_vocab.hip, gemm_store32.hip), as gemm_as.hip's entry
// points and beam_sparse.hip call them.
extern "C" int care_vocab32_applies(int M, int N, int K, int a_dtype, int has_labels);
extern "C" int care_vocab32_ranges(int M, int N, int min_parts);
extern "C" int care_vocab32_launch(const void* A, int64_t lda, const void* W, float* pmax, int32_t* pidx, float* psum,
                                   int M, int N, int ns, void* stream);
extern "C" int care_vocab32_launch_tiles(const void* A, int64_t lda, const void* W, float* pmax, int32_t* pidx, float* psum,
                                         float* tile_max, int M, int N, int ns, void* stream);
extern "C" int care_collect32_launch(const void* A, int64_t lda, const void* W, const float* thr, int32_t* cnt, float* cval,
                                     int32_t* cidx, int cap, int M, int N, int ns, void* stream);
extern "C" int care_store32_applies(int M, int N, int K, int a_dtype, int n_split, int has_bias_cols);
extern "C" int care_store32_launch(const void* A, int64_t lda, const void* W, const float* bias, void* C0, int64_t ldc0,
                                   int c0_bf16, void* C1, int64_t ldc1, int c1_bf16, int n_split, int M, int N, int act,
                                   void* stream);

// Launch of a 256-row kernel over the (panel, column range) items of p (M and ns set): one persistent workgroup of 512
// per CU (128 KiB or more of LDS each), at most 256 of them.
template <auto KERNEL, class P>
static inline int gs_launch256(P& p, int lds_bytes, void* stream) {
  p.panels = (p.M + GS_ROWS256 - 1) / GS_ROWS256;
  p.total_items = p.panels * p.ns;
  static std::atomic<unsigned long long> lds_ok{0};
  if (const int e = care_allow_dynamic_lds(reinterpret_cast<const void*>(KERNEL), lds_bytes, lds_ok)) return e;
  const int blocks = p.total_items < 256 ? p.total_items : 256;
  hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(512), lds_bytes, (hipStream_t)stream, p);
  return care_launch_status();
}
