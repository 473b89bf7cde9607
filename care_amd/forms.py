"""Which kernels a pass runs: DESIGN.md 5 ("Forms of the decode by batch size") as ONE function.

`plan(m, clips, bm, need, ...)` decides every form of a pass from the shape it STARTS with and returns a frozen `PassPlan`;
the engine keeps it as `engine.plan` for the length of the pass, the step code reads its fields, and every graph key
carries it (`graph_key`).  A clip's arithmetic must not change when compaction shrinks the row count mid-pass (DESIGN.md 7,
batch-size independence): nothing in a pass decides a form again from the current row count - except `mid_tile`, whose two
kernels are bit-identical.

`m` is the engine, read for
  * model facts: d, ff, H, V, T, Lk, n_layers, pre_ln, attr_att, topk, has_concepts, and the compute mode's as_ok / bf_act /
    bf / latent_ok / lean_ok;
  * limits, plain attributes that tests and tools set to force a form: latent, lanes, early_exit, resident_max_rows,
    resident_beam_max_rows, chain_beam_max_rows, BEAM_FUSED_MIN_ROWS, LATENT_MIN_ROWS;
  * the device: `_cus` (compute units; None without a device) and `_resident_refused` (row counts at which this device
    refused a resident launch).
Nothing here touches device memory or launches anything: it runs on the CPU (tests/test_forms_cpu.py holds every hand-over).
"""
import dataclasses
from typing import Optional

# ---------------------------------------------------------------------------------------------- thresholds
# K = 512 products between these row counts run on the LDS-tiled kernel: the A-stationary kernel's 128 / 256-row panels
# leave most of the chip idle there.  *measured* (round 5, tools/greedy_sweep.py / beam_sweep.py with the A-stationary / the
# LDS-tiled kernel forced, us per decoder step of the whole pass): greedy 512 clips 137 / 141, 1024 166 / 167, 2048 248 / 232,
# 4096 365 / 339, 8192 590 / 568; beam 5 over 256 clips (1280 rows) 284 / 272, 512 357 / 315, 1024 528 / 496, 2048 (10240 rows)
# 732 / 700; at 20480 rows the pass does not move and at 32768 the A-stationary kernels win in situ
MID_TILE_ROWS = (1280, 16384)
# small batches (the resident decodes): frame rows from which the embedder runs as the fused loader-wave kernel instead
# of GEMM + LayerNorm launches side by side (*measured* whole pass, fused / unfused: 64 clips 1.709 / 1.652 ms, 128 clips 1.809 /
# 1.803, 256 clips 2.637 / 2.689: from 192 clips)
FUSED_SMALL_MIN_ROWS = 5376
# up to this many rows the vocabulary arg-max of a d_model <= 512 model runs on the LDS-tiled kernel too (*measured* crossover
# between 2048 and 4096 rows on msrvtt_base_ami: 2048 rows 246 -> 241 us / step, 4096 rows 346 -> 356)
VOCAB_TILE_MAX_ROWS = 2048
# dense -> (+ residual) -> LayerNorm as ONE kernel (csrc/gemm_ln.hip) from this many rows: enough 64-row panels to occupy
# the chip; below, the A-stationary GEMM + LayerNorm kernel pair is faster.  *measured* (Base `ami`, whole pass): 8192 rows
# 435 K captions/s unfused vs 420 K fused, 12288 rows 440 K vs 446-451 K
LN_FUSED_MIN_ROWS = 10240
# Unfused FFN2 (K = ff) from this many rows on the LDS-tiled kernel (one product over the whole K, no slabs) instead of
# the split-K slabs of the A-stationary kernel
FFN2_TILE_MIN_ROWS = 1 << 30
# the cross-attention's d x d query projection (16-bit output) on the LDS-tiled kernel from this many rows (*measured* in
# situ, 32768 rows: 25.3 against 32-34 us on the A-stationary one, which wins the wider QKV / FFN1 products)
Q_TILE_MIN_ROWS = 8192
# LATENT_MIN_ROWS > 1 restores a row threshold of the absorbed cross-attention (tuning only; see `latent`)
LATENT_MIN_ROWS = 1
# Rows (clips x beam) from which the per-row top-k of beam search runs as two passes of the vocabulary GEMM on the
# 256-row panels (statistics -> threshold -> sparse collect -> pick: no [rows, V] logits in memory).  Below it the
# 16-bit modes take ONE pass of the LDS-tiled kernel that keeps group maxima (`beam_groups`; round 5), fp32 mode and
# beam sizes above 8 the materialised logits + care_beam_select.  All forms pick the same columns in the same order
# (tests/test_gpu_kernels.py::test_fused_beam_selection_..., test_beam_selection_from_group_maxima_...).
# *Measured* round 5 (beam 5, us per step of the whole pass, groups / two-pass): 5120 rows 422 / 497, 10240 rows 726 /
# 700, 20480 rows 1266 / 1162 - the group maxima are 12 KB per row and step.
BEAM_FUSED_MIN_ROWS = 8192
# Beam selection below BEAM_FUSED_MIN_ROWS in the 16-bit modes (beam_size <= 8): the vocabulary product on the LDS-tiled
# kernel keeping per (row, 64-column part) the maximum, sum exp and the maxima of its sixteen 4-column groups
# (care_gemm_tile_beam), then one wave per row picks the bm best groups and recomputes their 4 bm logits
# (care_beam_pick_groups) - two launches and 12 KB per row instead of the [rows, V] fp32 logits written and read back
# (*measured* round 5, beam 5, us per step of the whole multi-launch pass, logits + care_beam_select / groups: 160 rows
# 183 / 175, 640 rows 229 / 213, 1280 rows 274 / 245, 2560 rows 320 / 284).
BEAM_GROUPS_MIN_ROWS = 1
RESIDENT_MAX_V = 64 * 64 * 4  # csrc/decode_resident.hip: 64 lanes x RES_NP column-group partials of 64 columns
RESIDENT_WIDE_MAX_ROWS = 128  # d_model 768 / 1024: the K-split forms only (csrc/decode_resident.hip, template D)
RESIDENT_BEAM_MAX = 8  # csrc/decode_resident.h RES_BMK: 5 in the launch's first instance, 8 in its second (decode_resident_beam_wide.hip)
# beam search of the d_model 768 / 1024 models as one resident launch up to this many rows (160 at d_model 1024).  *Measured*
# (round 5, tools/beam_sweep.py, us per step of the whole pass, resident / multi-launch): d_model 1024 - 5 rows 103 / 207, 40
# rows 131 / 214, 125 rows 171 / 225, 160 rows 196 / 225, 200 rows 232 / 228; d_model 768 - 5 rows 88 / 186, 160 rows 152 / 202,
# 255 rows 183 / 207
RESIDENT_WIDE_BEAM_MAX_ROWS = 256


# ---------------------------------------------------------------------------------------------- one decision each
def resident_model_ok(m) -> bool:
    """Every model-side limit care_decode_resident / care_decode_resident_beam enforce (CARE_ESHAPE otherwise):
    16-bit mode; a post-LN decoder (the resident phases normalise AFTER the residual sum); d_model 512 (ff 512 / 1024 /
    2048), or d_model 768 / 1024 with ff = 4 d_model."""
    if m.pre_ln or not (m.bf and m.wt == m.h16 and m.T <= 128 and m.n_layers <= 4 and (not m.attr_att or m.topk <= 128) and
                        m.V <= RESIDENT_MAX_V and m.Lk <= 128):
        return False
    if m.d == 512:
        return bool(m.as_ok and m.ff in (512, 1024, 2048))
    return bool(m.d in (768, 1024) and m.ff == 4 * m.d and m.bf_act)


def resident_fits(m, kind: str, rows: int, per_tile: int = 1) -> bool:
    """One workgroup per CU at most, and at least one per group of `per_tile` 16-row tiles (a partitioned GPU has fewer
    CUs) - and below the smallest row count at which this device refused a resident launch of `kind` (CARE_ESHAPE: fewer
    co-resident workgroups than the launch needs; launches below it are still tried, the chained step never looks here)."""
    if rows >= m._resident_refused.get(kind, 1 << 30):
        return False
    return m._cus is None or ((rows + 15) // 16 + per_tile - 1) // per_tile <= m._cus // 8 * 8


def resident_greedy(m, clips: int) -> bool:
    """Greedy decode of `clips` clips as one resident launch (csrc/decode_resident.hip)?  A form of its own next to the
    multi-launch one: projected cross K/V, the same rounding points, sums in another order - so which of two nearly tied
    tokens wins can differ between a batch of <= resident_max_rows clips and a larger one (the audit of
    tests/test_gpu_properties.py counts such rows)."""
    return bool(0 < clips <= m.resident_max_rows and resident_model_ok(m) and (m.d == 512 or clips <= RESIDENT_WIDE_MAX_ROWS) and
                resident_fits(m, "greedy", clips))


def _beam_model_ok(m, bm: int, need: int, max_bm: int) -> bool:
    """The limits of care_decode_resident_beam: the greedy launch's, beam_size <= max_bm, a hypothesis' positions one per lane."""
    return bool(1 < bm <= max_bm and need >= 1 and resident_model_ok(m) and m.T <= 63 and m.V >= 16 * RESIDENT_BEAM_MAX)


def resident_beam(m, clips: int, bm: int, need: int) -> bool:
    """Beam search over `clips` clips as one resident launch (csrc/decode_resident_beam.hip)?"""
    rows = clips * bm
    if not (0 < rows <= m.resident_beam_max_rows and _beam_model_ok(m, bm, need, RESIDENT_BEAM_MAX)):
        return False
    if m.d != 512 and rows > (RESIDENT_WIDE_BEAM_MAX_ROWS if m.d <= 768 else min(160, RESIDENT_WIDE_BEAM_MAX_ROWS)):
        return False  # (d_model 768 / 1024: the K-split forms; see RESIDENT_WIDE_BEAM_MAX_ROWS)
    # (care_decode_resident_beam packs two row tiles per workgroup only in its forms for MORE than 512 rows; up to 512
    # rows it needs a workgroup per 16-row tile - a partitioned device with fewer CUs than tiles must not be promised
    # the resident form: ADVICE r4)
    return resident_fits(m, "beam", rows, 2 if rows > 512 else 1)


def chain_beam(m, clips: int, bm: int, need: int) -> bool:
    """Beam search over `clips` clips with every step a chain of kernels (csrc/decode_chain.hip)?  The model-side
    limits of the resident beam launch (its phases are the chain's kernels; RES_BMK of decode_chain.hip is 5, d_model 512);
    no residency condition, so the row count is bounded only by where the large-batch forms take over (`chain_beam_max_rows`)."""
    return bool(0 < clips * bm <= m.chain_beam_max_rows and m.d == 512 and _beam_model_ok(m, bm, need, 5))


def small_forms(m, clips: int) -> bool:
    """Batches of <= resident_max_rows clips (16-bit, d_model = 512) take the small-batch forms of the pass: the
    embedder as GEMM + LayerNorm launches side by side per modality (encode(small=True)) and, for greedy decoding,
    the resident decode.  `resident_max_rows = 0`: one set of forms at every batch size."""
    return bool(0 < clips <= m.resident_max_rows and m.as_ok and m.d == 512)


def latent(m, rows: int) -> bool:
    """Absorbed cross-attention for a multi-launch decode over `rows` rows?  The FORM OF THE ARITHMETIC is a
    property of the model and its compute mode (16-bit, d_model = 512 / 768 / 1024: absorbed; otherwise projected
    K/V), NOT of the batch a clip happens to be in: the two forms are two bf16 roundings of the same
    algebra, and switching between them by row count (round 1: from 2048 rows) made a clip's
    caption depend on the size of its batch wherever two tokens were nearly tied.  The price: the
    absorbed form has two more launches per step, which small, launch-bound batches feel
    (*measured* round 1: -15% at 32 rows, -1% at 1024; +5% at 2048, +13% at 16384).
    `engine.latent = False` (CARE_LATENT=0) selects projected K/V for every size instead.  The two exceptions, bought with
    the small-batch step rate: the resident decodes (projected K/V inside the launch) and beam search over a small batch
    (`PassPlan.small_beam`); `resident_max_rows = 0` restores one form at every size."""
    return bool(m.latent_ok and rows >= m.LATENT_MIN_ROWS)


def fuse_ln(m, rows: int) -> bool:
    """dense -> (+res) -> LayerNorm as ONE kernel (csrc/gemm_ln.hip): 16-bit mode, d_model = 512, a post-LN decoder."""
    return bool(m.as_ok and m.d == 512 and not m.pre_ln and rows >= LN_FUSED_MIN_ROWS)


def vocab_as(m, rows: int) -> bool:
    """The A-stationary vocabulary kernel (against the LDS-tiled one)?"""
    return bool(m.as_ok and rows > VOCAB_TILE_MAX_ROWS)


def mid_tile(rows: int) -> bool:
    """K = 512 products of `rows` rows on the LDS-tiled kernel (MID_TILE_ROWS).  The two kernels add K in the same order:
    BIT-IDENTICAL outputs (tests/test_gpu_kernels.py::test_tile_and_a_stationary_gemm_agree_bit_for_bit), so engine.gemm
    alone asks this by the CURRENT row count of every product - it changes no caption."""
    return MID_TILE_ROWS[0] <= rows < MID_TILE_ROWS[1]


def beam_fused(m, rows: int) -> bool:
    return bool(m.as_ok and rows >= m.BEAM_FUSED_MIN_ROWS)


def beam_groups(m, rows: int, bm: int) -> bool:
    return bool(m.bf_act and not beam_fused(m, rows) and bm <= 8 and rows >= BEAM_GROUPS_MIN_ROWS and
                128 <= m.V <= 16384 and m.d % 64 == 0)


def tf_fast(m, t: int, want_aux: bool) -> bool:
    """Teacher-forced forward on the fast kernels (_decode_full_fast): 16-bit mode, d_model = 512, no auxiliary
    dict entries (attention probabilities etc. are not materialised by the fused kernels)."""
    return bool(m.as_ok and m.d == 512 and not want_aux and t <= 32 and not m.pre_ln)


def lanes(m, clips: int) -> int:
    """Batch lanes of a graph-replayed greedy pass.

    A pass alternates HBM-bound kernels (attention, 44% of the time at B = 16384) with
    MFMA-bound ones (the GEMMs); two half-batches on two HIP streams inside the one captured
    graph let the one kind fill the other's idle unit and hide every kernel's tail.  Measured
    (bf16 Base `ami`, one MI355X): +8% at B = 4096, +5% at 8192/16384; at B <= 2048 the
    kernels are too short and the extra graph edges cost more than they hide (-3%..-30%), and
    4 lanes are never better than 2.

    A tuning knob, OFF by default (`engine.lanes` = 1; `engine.lanes = 2` turns it
    on): with two lanes the kernels share the chip, so per-kernel durations - and with them the
    roofline accounting of bench.py and profiles/ - no longer describe a kernel on its own.
    """
    return max(1, min(int(m.lanes), clips))


# ---------------------------------------------------------------------------------------------- the plan of a pass
@dataclasses.dataclass(frozen=True)
class PassPlan:
    """What a pass decided from its INITIAL shape.  Frozen and hashable: part of every graph key."""
    decode: str                # "resident" (one launch for all steps) | "chain" (beam: kernels chained per step) | "multi"
    clips: int
    bm: Optional[int]          # beam size of a beam search (translate_beam; 1 is a beam search too); None: greedy / teacher forcing
    need: int                  # hypotheses a clip collects before it is done
    rows: int                  # rows of a decoder step: clips x beam (teacher forcing: sequences x positions)
    small: bool                # the embedder's small-batch forms (encode(small=True))
    small_beam: bool           # beam search over a small batch: projected cross K/V (two launches less per step than the absorbed
                               # form, the beams of a clip share its K/V rows in cache; *measured* 128 clips x 5: 5.97 -> 5.47 ms
                               # per pass) and four waves per row in care_beam_select
    latent: bool               # absorbed cross-attention (`latent`)
    fuse_ln: bool              # dense + residual + LayerNorm in one kernel (`fuse_ln`)
    vocab_as: bool             # vocabulary arg-max on the A-stationary kernel (`vocab_as`)
    q_tile: bool               # the absorbed form's d x d query projection on the LDS-tiled kernel (Q_TILE_MIN_ROWS)
    mid_tile: bool             # `mid_tile` of the step's products at the initial row count (bit-identical kernels: see there)
    beam_select: str           # per-row top-k of beam search: "fused" (two passes) | "groups" (group maxima) | "logits"; "" without one
    sparse_second_pass: bool   # fused selection: second pass over the (tile, row) products that reach the row's threshold only
                               # (csrc/beam_sparse.hip; the library still refuses row counts its statistics kernel does not cover)
    lean: bool                 # the encoder writes the 16-bit memory alone (engine.lean_ok)
    early_exit: bool           # stop once every clip has ended; segments + compaction in the multi-launch forms
    lanes: int                 # batch lanes of a graph-replayed greedy pass (every lane plans its own rows)


def plan(m, clips: int, bm: Optional[int] = None, need: int = 1, lean: bool = False, early_exit: Optional[bool] = None,
         rows: Optional[int] = None, n_lanes: int = 1) -> PassPlan:
    """The plan of a pass over `clips` clips: greedy (bm None) or beam search of size bm.  `rows`: what a decoder step sees
    where it is not clips x beam (teacher forcing: sequences x positions; an ensemble member: the shared search's rows) -
    such a pass runs the multi-launch forms.  `n_lanes`: lanes_for(clips) of a graph-replayed greedy pass."""
    beam = bm is not None
    ee = bool(m.early_exit if early_exit is None else early_exit)
    decode = "multi"
    if rows is None and n_lanes == 1:
        if resident_beam(m, clips, bm, need) if beam else resident_greedy(m, clips):
            decode = "resident"
        elif beam and chain_beam(m, clips, bm, need):
            decode = "chain"
    rows = clips * (bm or 1) if rows is None else rows
    small, multi = small_forms(m, clips), decode != "resident"
    fused = beam and multi and beam_fused(m, rows)
    return PassPlan(
        decode=decode, clips=clips, bm=bm, need=need, rows=rows,
        small=(beam and not multi) or (small and (beam or not multi)), small_beam=beam and small,
        latent=latent(m, rows) and not (beam and small), fuse_ln=fuse_ln(m, rows), vocab_as=vocab_as(m, rows),
        q_tile=m.d == 512 and rows >= Q_TILE_MIN_ROWS, mid_tile=mid_tile(rows),
        beam_select=("fused" if fused else "groups" if beam_groups(m, rows, bm) else "logits") if beam and multi else "",
        sparse_second_pass=fused and m.d == 512, lean=bool(lean and m.lean_ok), early_exit=ee and n_lanes == 1, lanes=n_lanes)


def graph_key(name: str, plan: PassPlan, feats=(), *site) -> tuple:
    """Key of a captured hipGraph: the kind, the plan, what is the site's own (segment bounds, buffer-set parity, ensemble
    members), then the caller's feature buffers (addresses and shapes).  No site lists form facts by hand."""
    return (name, plan) + site + (tuple(f.data_ptr() for f in feats), tuple(tuple(f.shape) for f in feats))
