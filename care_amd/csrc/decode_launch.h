// decode_launch.h - HOST side of the resident and chained decodes (decode_resident.hip: greedy; decode_resident_beam.hip
// and its second instance decode_resident_beam_wide.hip: beam search; decode_chain.hip: beam steps as chained kernels).
// Every rule of the family is stated here ONCE: what a call must satisfy and which CARE_E* code it gets, the model part of
// RArgs, the scratch layout (size AND pointers), the vocabulary partials of a grid, the launch sequence.  The .hip files keep
// their own limits, grids and choice of a kernel instance.  Include after the device code of the translation unit.
#pragma once
#include "decode_resident.h"

constexpr int RES_MAX_ATT = 2;  // static-key attention blocks per layer (cross + attribute)
static_assert(sizeof(care_resident_layer::att) / sizeof(care_resident_attn) == RES_MAX_ATT &&
                  sizeof(RLayer::att) / sizeof(RAttn) == RES_MAX_ATT,
              "care_resident_layer::att / RLayer::att hold RES_MAX_ATT blocks");
// a step's phases (per layer: QKV, self-attention, dense, 3 per static-key block, FFN dense1, dense2; then vocabulary and
// beam advance) take the hand-off slots from 0 up and must stay below the init phase's slot, RES_MAX_SLOTS - 1
static_assert(RES_MAX_LAYERS * (5 + 3 * RES_MAX_ATT) + 2 <= RES_MAX_SLOTS - 1, "hand-off slots of a step reach the init phase's");

extern std::atomic<int> care_res_dbg_prof, care_res_dbg_ghost;  // decode_resident.hip (care_decode_resident_debug)
extern std::atomic<int> care_res_fenced_mode;                   // decode_resident.hip (care_resident_set_fenced): -1 auto, 0, 1

namespace {

// (res_zero_kernel: decode_resident.h - why a kernel and not hipMemsetAsync)
inline hipError_t res_zero_words(unsigned* p, int bytes, hipStream_t st) {
  hipLaunchKernelGGL(res_zero_kernel, dim3((bytes / 4 + 255) / 256), dim3(256), 0, st, p, bytes / 4);
  return hipGetLastError();
}

// care_resident_layer[] -> RArgs::L; 0 or a CARE_E* code
inline int res_fill_layers(RArgs& p, const care_resident_layer* layers, int n_layers) {
  for (int l = 0; l < n_layers; ++l) {
    const care_resident_layer& s = layers[l];
    RLayer& L = p.L[l];
    if (!s.qkv_w || !s.qkv_b || !s.o_w || !s.o_b || !s.ln_g || !s.ln_b || !s.self_kv || !s.w1 || !s.b1 || !s.w2 || !s.b2 ||
        !s.ffn_g || !s.ffn_b || s.n_att < 0 || s.n_att > RES_MAX_ATT)
      return CARE_EINVAL;
    L.qkv_w = (const bf16_t*)s.qkv_w; L.qkv_b = s.qkv_b; L.o_w = (const bf16_t*)s.o_w; L.o_b = s.o_b; L.g = s.ln_g; L.be = s.ln_b;
    L.skv = (bf16_t*)s.self_kv;
    L.n_att = s.n_att;
    for (int a = 0; a < s.n_att; ++a) {
      const care_resident_attn& sa = s.att[a];
      if (!sa.q_w || !sa.q_b || !sa.o_w || !sa.o_b || !sa.ln_g || !sa.ln_b || !sa.kv || sa.rows_per_kv < 1) return CARE_EINVAL;
      if (sa.nkeys < 1 || sa.nkeys > 8 * RES_MAXKB) return CARE_ESHAPE;
      RAttn& A = L.att[a];
      A.q_w = (const bf16_t*)sa.q_w; A.q_b = sa.q_b; A.o_w = (const bf16_t*)sa.o_w; A.o_b = sa.o_b; A.g = sa.ln_g; A.be = sa.ln_b;
      A.kv = (const bf16_t*)sa.kv; A.kv_bs = sa.kv_batch_stride; A.nkeys = sa.nkeys; A.rows_per_kv = sa.rows_per_kv;
      A.bias = sa.bias; A.bias_ld = sa.bias_ld;
    }
    L.w1 = (const bf16_t*)s.w1; L.b1 = s.b1; L.w2 = (const bf16_t*)s.w2; L.b2 = s.b2; L.fg = s.ffn_g; L.fbe = s.ffn_b;
  }
  p.n_layers = n_layers;
  return 0;
}

// Which hand-off a resident launch on the current device takes: the fence-free one only where it was validated
// (tests/test_gpu_resident.py's stress / contention tests run on gfx950 with all 256 CUs in one partition); any other
// device, partition mode or an explicit care_resident_set_fenced(1) / CARE_RESIDENT_FENCED=1 gets the release / acquire
// pair.  care_resident_set_fenced(0) forces the fence-free form (the validated arch is still a compile-time condition).
inline int res_fenced_for_device() {
  int mode = care_res_fenced_mode.load();
  if (mode < 0) {
    static const int env = [] { const char* e = getenv("CARE_RESIDENT_FENCED"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }();
    mode = env;
  }
  if (mode >= 0) return mode;
  // decided once per device ordinal (hipGetDeviceProperties is a driver round trip in front of a latency-bound launch)
  static std::atomic<int> per_device[64];
  static const bool init = [] { for (auto& a : per_device) a.store(-1); return true; }();
  (void)init;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  if (dev >= 0 && dev < 64) {
    const int known = per_device[dev].load(std::memory_order_relaxed);
    if (known >= 0) return known;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 1;
  const bool gfx950 = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
  const int fenced = (gfx950 && prop.multiProcessorCount == 256) ? 0 : 1;
  if (dev >= 0 && dev < 64) per_device[dev].store(fenced, std::memory_order_relaxed);
  return fenced;
}

// Tuning / tool / test knobs of the family: the environment is read ONCE per process (first launch), the debug hooks are
// set through care_decode_resident_debug (tests, tools/resident_prof.py), never through the environment.
struct ResKnobs {
  int rb, small, half_rows, beam_cfg, chain_cfg, chain_shared_min;  // -1: not set
  ResKnobs() {
    auto geti = [](const char* n) { const char* e = getenv(n); return e ? atoi(e) : -1; };
    rb = geti("CARE_RESIDENT_RB"); small = geti("CARE_RESIDENT_SMALL"); half_rows = geti("CARE_RESIDENT_HALF_ROWS");
    beam_cfg = geti("CARE_RESIDENT_BEAM_CFG"); chain_cfg = geti("CARE_CHAIN_CFG"); chain_shared_min = geti("CARE_CHAIN_SHARED_MIN_ROWS");
  }
};
inline const ResKnobs& res_knobs() {
  static const ResKnobs k;
  return k;
}

// The model and the workspace of a call, as every entry point of the family takes them.
struct ResModel {
  const care_resident_layer* layers; int n_layers;
  const float *word, *pos, *sem, *emb_g, *emb_b; float eps;
  const void* vocab_w; int V, d, heads, ff, act, T, stride;
  void* scratch; int64_t scratch_bytes;
};

// The checks every entry point makes, in the order that decides the code of a call that breaks several rules: null
// pointers, ranges (CARE_EINVAL), shapes (CARE_ESHAPE), activation (CARE_EDTYPE), workspace (CARE_EINVAL).  The entry
// point's own rules of a class arrive evaluated (state_ok: its state pointers; ranges_ok; limits_ok) and count at the
// position of their class; need_bytes is its *_scratch size.  0 or the code.
inline int res_check(const ResModel& m, bool state_ok, bool ranges_ok, bool limits_ok, int64_t need_bytes) {
  if (!m.layers || !m.word || !m.pos || !m.emb_g || !m.emb_b || !m.vocab_w || !state_ok || !m.scratch) return CARE_EINVAL;
  if (m.n_layers < 1 || m.n_layers > RES_MAX_LAYERS || m.T < 1 || m.V < 1 || m.stride < m.T + 1 || !ranges_ok) return CARE_EINVAL;
  // d_model 512 with ff 512 / 1024 / 2048, or 768 / 1024 with ff = 4 d_model (the kernels' D and KCF)
  const bool ff_ok = m.d == 512 ? (m.ff == 512 || m.ff == 1024 || m.ff == 2048) : ((m.d == 768 || m.d == 1024) && m.ff == 4 * m.d);
  if (m.heads * 64 != m.d || m.V > 64 * 64 * RES_NP || !ff_ok || !limits_ok) return CARE_ESHAPE;
  if (m.act < CARE_ACT_NONE || m.act > CARE_ACT_GELU) return CARE_EDTYPE;
  if (m.scratch_bytes < need_bytes || !care_aligned16(m.scratch)) return CARE_EINVAL;
  return 0;
}

// The model part of RArgs and its layers (res_fill_layers' code).  handoffs: a resident launch - the debug hooks
// (tools: phase clocks of step prof_step -> scratch + 2048; tests: ghost producers that never arrive, for the watchdog)
// and the form of the hand-off; the chained kernels have none.
inline int res_fill(RArgs& p, const ResModel& m, int sem_div, int rows, int steps, int bos, int eos, int pad, int early,
                    bool handoffs) {
  p.word = m.word; p.pos = m.pos; p.sem = m.sem; p.sem_div = sem_div; p.emb_g = m.emb_g; p.emb_be = m.emb_b; p.eps = m.eps;
  p.vocab = (const bf16_t*)m.vocab_w; p.V = m.V;
  p.d = m.d; p.H = m.heads; p.ff = m.ff; p.act = m.act; p.R = rows; p.T = m.T; p.steps = steps; p.bos = bos; p.eos = eos; p.pad = pad;
  p.early = early;
  p.prof_step = handoffs ? care_res_dbg_prof.load() : 0;
  p.ghost = handoffs && care_res_dbg_ghost.load() ? 8 : 0;
  p.fenced = handoffs ? res_fenced_for_device() : 0;
  return res_fill_layers(p, m.layers, m.n_layers);
}

// The stride of the vocabulary partials in the workspace = the most column items of the vocabulary phase a row can have
// (16 columns each when d_model > 512), capped at the partials the selection reads per lane.
inline int64_t res_max_parts(int d, int V) {
  const int64_t parts = d == 512 ? (V + 63) / 64 : (V + 15) / 16;
  return parts < 64 * RES_NP ? parts : 64 * RES_NP;
}

// THE layout of the workspace, for rows rounded up to whole 16-row tiles (R16):
//   sync | xres, y, y2, q fp32 [R16, d] | ctx bf16 [R16, d] | h bf16 [R16, ff] | pmax, pidx, psum [R16, parts]
//   beam: | gval, ggid [R16, parts, RES_BMK] | hn bf16 [R16, d] | xa bf16 [R16, d]
// Returns its bytes; with p, also sets p's pointers into `base`.  (The engine reads scratch[8:12], tools/resident_prof.py
// scratch + 2048: both inside sync.)
inline int64_t res_layout(RArgs* p, unsigned char* base, int64_t rows, int d, int ff, int V, bool beam) {
  const int64_t R16 = (rows + 15) / 16 * 16, parts = res_max_parts(d, V);
  RArgs sized_only;
  RArgs& a = p ? *p : sized_only;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { off += bytes; return p ? base + off - bytes : nullptr; };
  a.sync = (unsigned*)take(RES_SYNC_BYTES);
  a.xres = (float*)take(R16 * d * 4); a.y = (float*)take(R16 * d * 4); a.y2 = (float*)take(R16 * d * 4); a.q = (float*)take(R16 * d * 4);
  a.ctx = (bf16_t*)take(R16 * d * 2);
  a.h = (bf16_t*)take(R16 * ff * 2);
  a.pmax = (float*)take(R16 * parts * 4); a.pidx = (int32_t*)take(R16 * parts * 4); a.psum = (float*)take(R16 * parts * 4);
  if (beam) {
    a.gval = (float*)take(R16 * parts * RES_BMK * 4); a.ggid = (int32_t*)take(R16 * parts * RES_BMK * 4);
    a.hn = (bf16_t*)take(R16 * d * 2);
    a.xa = (bf16_t*)take(R16 * d * 2);
  }
  return off;
}

inline int res_device_cus(int& cus) {  // CUs of the current device; 0 or the hipError_t
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return e == hipSuccess ? 0 : (int)e;
}

// vocabulary partials per row of a grid: workgroups per row group that have a column item (PhaseMap)
inline int res_parts(int grid, int RG, int CIV) {
  const int nper = ((grid & 7) == 0 && (grid >> 3) >= RG) ? 8 * ((grid >> 3) / RG) : grid / RG;
  return nper < CIV ? nper : CIV;
}

// Every workgroup of a resident launch must be resident at the same time: the grid is at most one workgroup per CU, and
// the occupancy query must admit one workgroup of this kernel per CU (registers, LDS).  0 or a CARE_E* / hipError_t code.
inline int res_check_residency(const void* kernel, int lds, int grid, int cus) {
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, (size_t)lds);
  if (e != hipSuccess) return (int)e;
  return (nb >= 1 && grid <= cus) ? 0 : CARE_ESHAPE;
}

// The launch of a resident kernel instance: raise its LDS limit (once per device), check residency (once per instance:
// `ok`) BEFORE anything is enqueued - a refused launch leaves the stream untouched -, zero the sync area, launch.
template <class K>
int res_launch(K kernel, std::atomic<unsigned long long>& lds_done, std::atomic<int>& ok, int lds, int grid, int cus, const RArgs& p,
               hipStream_t st) {
  const void* kfn = (const void*)kernel;
  if (const int rc = care_allow_dynamic_lds(kfn, lds, lds_done)) return rc;
  if (!ok.load(std::memory_order_acquire)) {
    if (const int rc = res_check_residency(kfn, lds, grid, cus)) return rc;
    ok.store(1, std::memory_order_release);
  }
  if (const hipError_t e = res_zero_words(p.sync, RES_SYNC_BYTES, st); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, p);
  return care_launch_status();
}

}  // namespace
