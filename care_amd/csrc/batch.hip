// batch.hip - a training / validation batch built on the device (include/care_hip.h, "Training and validation batches built on
// the device"; care_amd/clipstore.py): frame ids per item from a counter-based generator, the feature rows of every modality
// gathered out of the per-video tables in HBM, and the caption of every item cut and padded into input_ids / labels with the
// video's concept labels.  Integer and byte arithmetic only: the same code in both library variants.
//
// The gather is the bandwidth path.  A 512-clip MSRVTT batch is 154 MB read and 154 MB written in rows of 512 B .. 8 KB that
// lie scattered over tables far larger than the Infinity Cache and are read once an epoch.  The unit of work is a PIECE: 1 KiB
// of one destination row (64 lanes x 16 B, one wave-instruction).  A wave takes BG_PIECES consecutive pieces of the launch's
// flat piece list, issues all their loads before the first store (4 KiB in flight per wave, 16 waves per CU: the shape
// MI355X measurements give for whole rows gathered into registers) and then stores them.  The tables of all modalities are
// one list in the kernel arguments (as csrc/optim.hip passes its tensors), so a batch is one launch.
#include "care_common.h"

namespace {

#define BST ((hipStream_t)stream)

// ---------------------------------------------------------------------------------------------------------------- frame ids
struct FrameBounds {
  int32_t b[CARE_BATCH_MAX_FRAMES + 1];
};
static_assert(sizeof(FrameBounds) <= 1024, "the bounds travel in the kernel arguments");

constexpr int BF_WAVES = 4;   // items of a workgroup: one wave each

__global__ __launch_bounds__(BF_WAVES * 64) void frame_ids_kernel(const int32_t* items, int B, int n_total, int n_frames, int type,
                                                                  const FrameBounds bd, unsigned long long seed,
                                                                  unsigned long long epoch, int32_t* out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * BF_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;   // (whole waves leave: the ballot below sees a full wave)
  int32_t* o = out + (int64_t)b * n_frames;
  if (type == CARE_FRAMES_EQUAL) {
    for (int i = lane; i < n_frames; i += 64) o[i] = (bd.b[i] + bd.b[i + 1]) / 2;
    return;
  }
  // (h = care_mix64: an item's frames depend on (seed, epoch, item) alone)
  const unsigned long long k1 = care_mix64(care_mix64(seed, epoch), (unsigned long long)(long long)items[b]);
  if (type == CARE_FRAMES_SEGMENT) {
    for (int i = lane; i < n_frames; i += 64) {
      const unsigned r = (unsigned)(care_mix64(k1, (unsigned long long)i) >> 32);
      const unsigned w = (unsigned)(bd.b[i + 1] - bd.b[i]);
      o[i] = bd.b[i] + (int)(((unsigned long long)r * w) >> 32);
    }
    return;
  }
  // CARE_FRAMES_ALL: n_total <= 64, frame `lane`.  Lanes at or beyond n_total hold no frame: they are never counted, and
  // rank = n_total keeps them out of the ballot.
  const unsigned long long key = care_mix64(k1, (unsigned long long)lane);
  const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
  int rank = 0;
  for (int g = 0; g < n_total; ++g) {
    const unsigned long long kg = ((unsigned long long)(unsigned)__shfl((int)khi, g, 64) << 32) | (unsigned)__shfl((int)klo, g, 64);
    rank += (kg < key || (kg == key && g < lane)) ? 1 : 0;
  }
  const bool chosen = lane < n_total && rank < n_frames;
  const unsigned long long mask = __ballot(chosen);
  if (chosen) o[__popcll(mask & ((1ull << lane) - 1ull))] = lane;
}

// ------------------------------------------------------------------------------------------------------------------ gather
constexpr int BG_PIECE = 1024;   // bytes of a piece: one 16-byte access per lane
constexpr int BG_PIECES = 4;     // pieces a wave has in flight
constexpr int BG_WAVES = 4;      // waves of a workgroup

struct GatherTable {
  const unsigned char* table; unsigned char* out;
  long long pitch;
  long long piece_end;           // the flat piece list: this table owns [piece_end of the table before, piece_end)
  int n_total, row_bytes, n_out, row_pieces;
};
struct GatherPack {
  GatherTable t[CARE_BATCH_MAX_TABLES];
  int count;
};
static_assert(sizeof(GatherPack) <= 1024, "the table list travels in the kernel arguments");

// UNIT: bytes of a store - 16 (rows of a multiple of 16 bytes into a 16-byte aligned output), 4 or 2
template <int UNIT>
__device__ __forceinline__ void bg_store(unsigned char* dst, const u32x4 v, int nbytes) {
  if (UNIT == 16) {
    *reinterpret_cast<u32x4*>(dst) = v;   // (nbytes is 16: the row is whole 16-byte units)
  } else if (UNIT == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * k < nbytes) reinterpret_cast<unsigned*>(dst)[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (2 * k < nbytes) reinterpret_cast<unsigned short*>(dst)[k] = (unsigned short)(v[k >> 1] >> (16 * (k & 1)));
  }
}

template <int UNIT>
__global__ __launch_bounds__(BG_WAVES * 64) void gather_kernel(const GatherPack pk, const int32_t* video_ids, const int32_t* frame_ids,
                                                               int n_videos, int n_frames, long long pieces) {
  const int lane = threadIdx.x & 63;
  // (the wave's number through readfirstlane: the piece, its table and its row are wave-uniform - scalar registers, and the
  // table list is read where it lies, in the kernel arguments)
  const long long p0 = ((long long)blockIdx.x * BG_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * BG_PIECES;
  u32x4 v[BG_PIECES];
  unsigned char* dst[BG_PIECES];
  int nb[BG_PIECES];
  bool ok[BG_PIECES];
  // No divergent branch around a load: every lane of every piece loads 16 bytes from an address that is always valid - its
  // own, or the table's first 16 bytes when it has nothing to read - so the four loads are in flight together and the
  // decision between the loaded bytes and zeros is taken at the store.
#pragma unroll
  for (int q = 0; q < BG_PIECES; ++q) {
    const bool live = p0 + q < pieces;
    const long long p = live ? p0 + q : pieces - 1;
    int ti = 0;
    long long base = 0;
    while (ti < pk.count - 1 && p >= pk.t[ti].piece_end) base = pk.t[ti++].piece_end;
    const GatherTable& t = pk.t[ti];
    const unsigned pt = (unsigned)(p - base);                 // (a table owns fewer than 2^31 pieces: care_batch_gather)
    const unsigned r = pt / (unsigned)t.row_pieces;           // destination row b * n_out + j
    const int piece = (int)(pt - r * (unsigned)t.row_pieces);
    const int b = (int)(r / (unsigned)t.n_out), j = (int)(r - (unsigned)b * (unsigned)t.n_out);
    const int off = piece * BG_PIECE + lane * 16;
    nb[q] = live ? min(16, t.row_bytes - off) : 0;            // <= 0: nothing of the row at this lane
    dst[q] = t.out + (long long)r * t.row_bytes + off;
    const int vid = video_ids[b];
    const int fr = (t.n_total == 1 ? video_ids : frame_ids)[t.n_total == 1 ? (long long)b : (long long)b * n_frames + j];
    const int f = t.n_total == 1 ? 0 : fr;
    // a video or frame id outside the table is never dereferenced: the row is zeros
    ok[q] = nb[q] > 0 && vid >= 0 && vid < n_videos && f >= 0 && f < t.n_total;
    // (the source row is 16-byte aligned and `pitch` - a multiple of 16 - long: the 16 bytes at `off` lie inside it)
    const unsigned char* src = t.table + (ok[q] ? ((long long)vid * t.n_total + f) * t.pitch + off : 0ll);
    v[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
  }
#pragma unroll
  for (int q = 0; q < BG_PIECES; ++q)
    if (nb[q] > 0) bg_store<UNIT>(dst[q], ok[q] ? v[q] : u32x4{0u, 0u, 0u, 0u}, nb[q]);
}

// -------------------------------------------------------------------------------------------------------------------- text
constexpr int BX_THREADS = 256;
constexpr int BX_WORDS = (CARE_BATCH_MAX_ATTR + 31) / 32;

struct TextArgs {
  const int32_t* items; const int32_t* item_cap; const int32_t* tokens; const int32_t* cap_start; const int32_t* cap_video;
  const int32_t* vid_first;
  int n_items, n_caps, n_videos, max_len, pad, eos, attr0, n_attr;
  int32_t* video_ids; int32_t* caption_ids; long long* input_ids; long long* labels; float* labels_attr;
};

__global__ __launch_bounds__(BX_THREADS) void text_kernel(const TextArgs a) {
  __shared__ unsigned bits[BX_WORDS];
  const int tid = threadIdx.x, b = blockIdx.x, W = a.max_len - 1;
  const int item = a.items[b];
  int c = -1, v = -1;
  if (item >= 0 && item < a.n_items) {
    c = a.item_cap[item];
    if (c < 0 || c >= a.n_caps) c = -1;
  }
  if (c >= 0) {
    v = a.cap_video[c];
    if (v < 0 || v >= a.n_videos) { v = -1; c = -1; }
  }
  if (tid == 0) {
    a.video_ids[b] = v;
    a.caption_ids[b] = c < 0 ? -1 : c - a.vid_first[v];
  }
  // _padding(target, add_eos = True) (dataloader.py:661-675), then source = [:-1], target = [1:] (:570-571)
  const int t0 = c < 0 ? 0 : a.cap_start[c];
  const int L = c < 0 ? 0 : a.cap_start[c + 1] - t0;
  for (int p = tid; p < a.max_len; p += BX_THREADS) {
    int tok = a.pad;
    if (p < L) tok = (L > a.max_len && p == a.max_len - 1) ? a.eos : a.tokens[t0 + p];
    if (p < W) a.input_ids[(long long)b * W + p] = tok;
    if (p > 0) a.labels[(long long)b * W + p - 1] = tok;
  }
  if (!a.labels_attr) return;
  // get_vid2attribute_mappings (misc/utils_corpora.py:424-441): every caption of the video, cap[1:-1]
  const int words = (a.n_attr + 31) / 32;
  for (int i = tid; i < words; i += BX_THREADS) bits[i] = 0u;
  __syncthreads();
  if (v >= 0) {
    const int c0 = a.vid_first[v], c1 = a.vid_first[v + 1];
    for (int cc = c0 + (tid >> 3); cc < c1; cc += BX_THREADS / 8) {   // eight lanes a caption
      const int s = a.cap_start[cc] + 1, e = a.cap_start[cc + 1] - 1;
      for (int p = s + (tid & 7); p < e; p += 8) {
        const int k = a.tokens[p] - a.attr0;
        if (k >= 0 && k < a.n_attr) atomicOr(&bits[k >> 5], 1u << (k & 31));
      }
    }
  }
  __syncthreads();
  float* o = a.labels_attr + (long long)b * a.n_attr;
  for (int k = tid; k < a.n_attr; k += BX_THREADS) o[k] = (bits[k >> 5] >> (k & 31)) & 1u ? 1.f : 0.f;
}

inline bool bt_al(const void* p, unsigned a) { return (((uintptr_t)p) & (a - 1u)) == 0; }

}  // namespace

extern "C" int care_batch_frame_ids(const int32_t* items, int B, int n_total, int n_frames, int random_type, const int32_t* bounds,
                                    uint64_t seed, uint64_t epoch, int32_t* frame_ids, void* stream) {
  const bool random = random_type != CARE_FRAMES_EQUAL;
  if (random_type != CARE_FRAMES_EQUAL && random_type != CARE_FRAMES_SEGMENT && random_type != CARE_FRAMES_ALL) return CARE_EDTYPE;
  if (!frame_ids || !bounds || (random && !items) || B < 0 || n_total < 1 || n_frames < 1) return CARE_EINVAL;
  if (n_frames > CARE_BATCH_MAX_FRAMES || (random && n_frames > n_total)) return CARE_ESHAPE;
  if (random_type == CARE_FRAMES_ALL && n_total > 64) return CARE_ESHAPE;
  if (!bt_al(frame_ids, 4) || (items && !bt_al(items, 4))) return CARE_EALIGN;
  FrameBounds bd = {};
  if (bounds[0] != 0 || bounds[n_frames] != n_total) return CARE_EINVAL;
  for (int i = 0; i <= n_frames; ++i) {
    if (i && (bounds[i] < bounds[i - 1] || (random && bounds[i] == bounds[i - 1]))) return CARE_EINVAL;
    bd.b[i] = bounds[i];
  }
  // (the middle of an empty last snippet would be n_total: equally_sampling with n_frames > n_total keeps every middle below it,
  // since an empty snippet [x, x) with x == n_total can only follow the last frame - checked here, not assumed)
  for (int i = 0; i < n_frames; ++i)
    if ((bd.b[i] + bd.b[i + 1]) / 2 >= n_total) return CARE_EINVAL;
  if (B == 0) return 0;
  hipLaunchKernelGGL(frame_ids_kernel, dim3((B + BF_WAVES - 1) / BF_WAVES), dim3(BF_WAVES * 64), 0, BST, items, B, n_total, n_frames,
                     random_type, bd, (unsigned long long)seed, (unsigned long long)epoch, frame_ids);
  return care_launch_status();
}

extern "C" int care_batch_gather(const care_batch_table* tables, int count, const int32_t* video_ids, const int32_t* frame_ids,
                                 int n_videos, int B, int n_frames, void* stream) {
  if (!tables || !video_ids || count < 1 || B < 0 || n_videos < 1 || n_frames < 1) return CARE_EINVAL;
  if (count > CARE_BATCH_MAX_TABLES) return CARE_ESHAPE;
  if (!bt_al(video_ids, 4) || (frame_ids && !bt_al(frame_ids, 4))) return CARE_EALIGN;
  GatherPack pk = {};
  pk.count = count;
  int unit = 16;
  long long pieces = 0;
  for (int i = 0; i < count; ++i) {
    const care_batch_table& s = tables[i];
    if (!s.table || !s.out || s.n_total < 1 || s.n_out < 1 || s.row_bytes < 2 || (s.row_bytes & 1) || s.pitch < s.row_bytes)
      return CARE_EINVAL;
    if (s.n_total > 1 && !frame_ids) return CARE_EINVAL;
    if (s.n_total > 1 && s.n_out != n_frames) return CARE_ESHAPE;
    if (!bt_al(s.table, 16) || (s.pitch & 15) || !bt_al(s.out, 2)) return CARE_EALIGN;
    const int u = ((s.row_bytes & 15) == 0 && bt_al(s.out, 16)) ? 16 : ((s.row_bytes & 3) == 0 && bt_al(s.out, 4)) ? 4 : 2;
    if (u < unit) unit = u;   // one launch, one store width: the narrowest any table needs
    GatherTable& t = pk.t[i];
    t.table = static_cast<const unsigned char*>(s.table);
    t.out = static_cast<unsigned char*>(s.out);
    t.pitch = s.pitch;
    t.n_total = s.n_total; t.row_bytes = s.row_bytes; t.n_out = s.n_out;
    t.row_pieces = (s.row_bytes + BG_PIECE - 1) / BG_PIECE;
    const long long own = (long long)B * s.n_out * t.row_pieces;
    if (own > 0x7FFFFFFFll) return CARE_ESHAPE;
    pieces += own;
    t.piece_end = pieces;
  }
  if (B == 0) return 0;
  const long long per_block = (long long)BG_WAVES * BG_PIECES;
  const long long grid = (pieces + per_block - 1) / per_block;
  if (grid > 0x7FFFFFFFll) return CARE_ESHAPE;
  if (unit == 16)
    hipLaunchKernelGGL(gather_kernel<16>, dim3((unsigned)grid), dim3(BG_WAVES * 64), 0, BST, pk, video_ids, frame_ids, n_videos, n_frames, pieces);
  else if (unit == 4)
    hipLaunchKernelGGL(gather_kernel<4>, dim3((unsigned)grid), dim3(BG_WAVES * 64), 0, BST, pk, video_ids, frame_ids, n_videos, n_frames, pieces);
  else
    hipLaunchKernelGGL(gather_kernel<2>, dim3((unsigned)grid), dim3(BG_WAVES * 64), 0, BST, pk, video_ids, frame_ids, n_videos, n_frames, pieces);
  return care_launch_status();
}

extern "C" int care_batch_text(const int32_t* items, int B, const int32_t* item_cap, int n_items, const int32_t* tokens,
                               const int32_t* cap_start, const int32_t* cap_video, const int32_t* vid_first, int n_caps, int n_videos,
                               int max_len, int pad, int eos, int attribute_start, int n_attributes, int32_t* video_ids,
                               int32_t* caption_ids, int64_t* input_ids, int64_t* labels, float* labels_attr, void* stream) {
  if (!items || !item_cap || !tokens || !cap_start || !cap_video || !vid_first || !video_ids || !caption_ids || !input_ids || !labels)
    return CARE_EINVAL;
  if (B < 0 || n_items < 1 || n_caps < 1 || n_videos < 1 || max_len < 2) return CARE_EINVAL;
  if (labels_attr && (n_attributes < 1 || n_attributes > CARE_BATCH_MAX_ATTR)) return CARE_ESHAPE;
  if (!bt_al(input_ids, 8) || !bt_al(labels, 8)) return CARE_EALIGN;
  const void* four[] = {items, item_cap, tokens, cap_start, cap_video, vid_first, video_ids, caption_ids, labels_attr};
  for (const void* p : four)
    if (p && !bt_al(p, 4)) return CARE_EALIGN;
  if (B == 0) return 0;
  TextArgs a;
  a.items = items; a.item_cap = item_cap; a.tokens = tokens; a.cap_start = cap_start; a.cap_video = cap_video; a.vid_first = vid_first;
  a.n_items = n_items; a.n_caps = n_caps; a.n_videos = n_videos; a.max_len = max_len; a.pad = pad; a.eos = eos;
  a.attr0 = attribute_start; a.n_attr = labels_attr ? n_attributes : 0;
  a.video_ids = video_ids; a.caption_ids = caption_ids;
  a.input_ids = reinterpret_cast<long long*>(input_ids); a.labels = reinterpret_cast<long long*>(labels); a.labels_attr = labels_attr;
  hipLaunchKernelGGL(text_kernel, dim3(B), dim3(BX_THREADS), 0, BST, a);
  return care_launch_status();
}
