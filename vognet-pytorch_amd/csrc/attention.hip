// K1: rel_attention_fwd — softmax((Q K^T + bias)/sqrt(d_model)) V per
// (sequence, head), flash-style on gfx950, with the reference's relative
// position bias recomputed per block instead of materialised.
//
// Replaces RelAttention.forward / Attention.forward (transformer_code.py:136-160,
// 42-50) and the whole of compute_pe (mdl_vog.py:456-490): the reference builds
// pe[S,N,N,H] = relu(Linear(5,H)(box_i - box_j)) (5.9 GB of temporaries at p100);
// the Linear is affine in the box, so pe[i,j,h] = relu(u[i,h] - u[j,h] + b[h])
// with u = W_pe . box — three VALU ops per (i,j), nothing stored.
//
// Eleven kernels share the math below and differ in how K / V reach the MFMA (csrc/attention_dev.h, attn_tile2_dev.h,
// attn_struct_lds_dev.h, attn_struct_ef_dev.h). vog_rel_attention_fwd (attn_plan below; DESIGN.md has the rules as a table):
// attn_sb (N <= 128: keys split over the 4 waves, global softmax statistics exchanged through LDS before P.V), attn_frag8 /
// attn_frag_lean (up to 8 key blocks: every operand requested in one round trip / the 128-register form, which also carries
// the hi + lo operands and out16_lo), attn_frag (more than 8 key blocks, N < 512: per-wave running softmax, LDS tree merge),
// attn_tile (N >= 512, and hi + lo operands beyond 8 key blocks: K / V^T blocks staged once per workgroup by LDS-DMA, double
// buffered) and attn_tile2 (N >= 1024 with a guard word, head dim <= 192: two waves per SIMD, fixed-reference softmax that
// raises the guard, attn_tile as the gated fallback pass). vog_rel_attention_struct_fwd (attn_struct_plan; mul_tx layer 0,
// separable softmax over visual + language keys): attn_struct1_dma / attn_struct1_lean (one visual key block), attn_struct_lds
// (several: K / V^T through an LDS ring), attn_struct_ef (the E x F factorisation, attn_struct_lds as its gated fallback) and
// attn_struct (several key blocks whose ring does not fit the LDS).
// Host side: validate the argument block, plan (a pure function: which kernels, grids, LDS), execute the plan.
// Common mapping (wave64, v_mfma_f32_32x32x16): a wave owns 32 queries;
//   * "swapped" products so a query's softmax row lives in one lane:
//       S^T[key][q] = K_blk . Q^T        (A = K fragment, B = Q fragment)
//       O^T[d][q]  += V^T_blk . P^T      (A = V fragment, B = P from registers)
//     C/D has col = lane&31 = query for both, so running max / sum / rescale are
//     per-lane scalars, and P goes from the S accumulator registers straight into
//     the B operand: the MFMA k index is a free summation index, so register r
//     of half hi is declared to be k = hi*8 + (r&7) of k-step r>>3 and V is stored
//     with the matching key permutation (common.h frag_v). No cross-lane
//     movement, no LDS round trip for P.
//   * q, k, v arrive in MFMA-fragment order (written that way by the QKV GEMM
//     epilogue / vog_qkv_combine): every operand fragment is one contiguous KiB,
//     loaded straight into registers (or, for attn_tile, into LDS by global_load_lds) with
//     16-byte-per-lane coalesced accesses: no transposes, no swizzles.
#include <type_traits>
#include "attention_dev.h"
#include "attn_tile2_dev.h"
#include "attn_struct_lds_dev.h"
#include "attn_struct_ef_dev.h"

namespace vog {

// ---- LDS: the limits raised per kernel family, and the dynamic bytes of every kernel -------------------------------------------
static constexpr size_t kCapLong = 150 * 1024;    // attn_frag, attn_tile, attn_struct_lds, attn_struct_ef; the budget of the hi + lo forms
static constexpr size_t kCapTile2 = 160 * 1024;   // attn_tile2
static constexpr size_t kCapSb = 80 * 1024;       // attn_sb
static constexpr size_t kCapDma = 72 * 1024;      // attn_struct1_dma
static constexpr size_t kCapPlain = 64 * 1024;    // attn_frag8; what the kernels without a raise (attn_struct1_lean, attn_struct) may use

// A key block in an LDS ring is K and V^T (dp / 16 + 2 * (dp / 32) KB); the hi + lo forms add the K remainders.
static constexpr size_t ring_block_bytes(int dp) { return (size_t)(dp / 16 + 2 * (dp / 32)) * 1024; }
static constexpr size_t split_block_bytes(int dp) { return (size_t)(2 * (dp / 16) + 2 * (dp / 32)) * 1024; }
static constexpr size_t attn_sb_lds(int dp, int npad) { return ((size_t)4 * ((dp / 32 + 1) / 2) * 16 * 64 + 4 * 2 * 64 + npad) * sizeof(float); }
static constexpr size_t attn_frag_lean_lds(int npad) { return (size_t)8 * 2 * 64 * 16 + (size_t)2 * 8 * 32 * sizeof(float) + (size_t)npad * sizeof(float); }
static constexpr size_t attn_frag8_lds(int dp, int npad) { return (size_t)(dp / 16 + 16) * 1024 + (size_t)2 * 8 * 32 * sizeof(float) + (size_t)npad * sizeof(float); }
static constexpr size_t attn_frag_lds(int dp, int npad) { return ((size_t)2 * (dp / 32) * 16 * 64 + 4 * 2 * 64 + npad) * sizeof(float); }
// attn_tile: two ring slots + one bias precursor per key; attn_tile2: four slots
static constexpr size_t attn_tile_lds(int dp, int npad, bool split) { return 2 * (split ? split_block_bytes(dp) : ring_block_bytes(dp)) + (size_t)npad * sizeof(float); }
static constexpr size_t attn_tile2_lds(int dp, int npad) { return 4 * ring_block_bytes(dp) + (size_t)npad * sizeof(float); }
// attn_struct_lds: four ring slots (hi + lo: two) + bias precursors + the language rows (nsrl x Q / K / V x dp floats)
static constexpr size_t attn_struct_lds_lds(int dp, int npad_kv, int nsrl, bool split) {
  return (split ? 2 * split_block_bytes(dp) : 4 * ring_block_bytes(dp)) + ((size_t)npad_kv + (size_t)nsrl * 3 * dp) * sizeof(float);
}
// attn_struct1_lean, attn_struct: bias precursors, and with one visual key block the language rows
static constexpr size_t attn_struct_row_lds(int dp, int npad_kv, int nsrl) {
  return npad_kv == 32 ? (size_t)(32 + nsrl * 3 * dp) * sizeof(float) : (size_t)npad_kv * sizeof(float);
}
static constexpr size_t attn_struct1_dma_lds(int dp, int nsrl) {
  return (size_t)(7 * (dp / 32)) * 1024 + (size_t)2 * (nsrl + 1) * dp * sizeof(unsigned short) + 32 * sizeof(float);
}

static const char* const kAttnKernelNames[VOG_ATTN_KERNELS] = {
    "attn_guard_clear_kernel", "attn_sb_kernel", "attn_frag_lean_kernel", "attn_frag8_kernel", "attn_frag_kernel", "attn_tile_kernel",
    "attn_tile2_kernel", "attn_struct1_lean_kernel", "attn_struct1_dma_kernel", "attn_struct_kernel", "attn_struct_lds_kernel",
    "attn_struct_ef_kernel"};

static bool head_dim_ok(int dp) { return dp == 32 || dp == 64 || dp == 128 || dp == 192 || dp == 256; }

// ---- plans ---------------------------------------------------------------------------------------------------------------------
// Pure host functions: no HIP call, only the scalar fields of the argument block and the null-ness of its optional pointers.
struct AttnPlan {
  int n = 0;
  vog_attn_launch l[3];
  void add(int kernel, int flag, int grid, int block, size_t lds, size_t cap, int guard = VOG_ATTN_GUARD_NONE) {
    l[n++] = vog_attn_launch{kernel, flag, (unsigned)grid, (unsigned)block, (unsigned)lds, (unsigned)cap, guard};
  }
};

// vog_rel_attention_fwd: [guard clear,] first pass [, gated fallback pass]
static int attn_plan(const vog_attn_args& a, AttnPlan& pl) {
  pl.n = 0;
  if (a.dtype != VOG_BF16 && a.dtype != VOG_F16) VOG_FAIL(-1, "unknown vog_dtype %d", (int)a.dtype);
  if (!head_dim_ok(a.dp)) VOG_FAIL(-1, "rel_attention: unsupported padded head dim %d (32/64/128/192/256)", a.dp);
  const int dp = a.dp, N = a.N, npad = a.npad, sh = a.H * a.S;
  const int g32 = ceil_div(N, 32) * sh, g128 = ceil_div(N, 128) * sh;      // one wave per 32 queries: 1 / 4 waves per workgroup
  const bool split = a.q_lo != nullptr;                                      // hi + lo Q / K: the three-MFMA contraction
  if (N <= 128) { pl.add(VOG_ATTN_SB_KERNEL, split, g32, 256, attn_sb_lds(dp, npad), kCapSb); return 0; }
  if (split) {
    if (npad <= 256) { pl.add(VOG_ATTN_FRAG_LEAN_KERNEL, 1, g32, 256, attn_frag_lean_lds(npad), 0); return 0; }
    // longer sequences (p100; gt5 spat with 6 or more videos per query): the running-maximum tile kernel with the K remainders
    // in its ring. No fixed-reference pass and no guard: logits that need this plan would raise the guard anyway.
    const size_t lds = attn_tile_lds(dp, npad, true);
    if (lds > kCapLong) VOG_FAIL(-1, "rel_attention with hi + lo operands: sequence of %d tokens exceeds the LDS budget", N);
    pl.add(VOG_ATTN_TILE_KERNEL, 1, g128, 256, lds, kCapLong);
    return 0;
  }
  // very long sequences: two waves per SIMD, fixed-reference softmax that raises the guard word (head dim 256 would spill);
  // the running-maximum tile kernel is its fallback pass, the only kernel that honours the word
  const bool tile2 = N >= 1024 && a.guard_flag && dp <= 192 && attn_tile2_lds(dp, npad) <= kCapTile2;
  // long sequences: enough 128-query groups to fill the chip -> shared K / V tiles through LDS
  if (N >= 512) {
    const size_t lds = attn_tile_lds(dp, npad, false);
    if (lds > kCapLong) VOG_FAIL(-1, "rel_attention: sequence of %d tokens exceeds the LDS budget", N);
    if (tile2) {
      // (the clear is a kernel, not a memset: graph-capturable on any stream)
      if (!a.guard_precleared) pl.add(VOG_ATTN_GUARD_CLEAR_KERNEL, 0, 1, 64, 0, 0, VOG_ATTN_GUARD_FLAG);
      pl.add(VOG_ATTN_TILE2_KERNEL, 0, ceil_div(N, 256) * sh, 512, attn_tile2_lds(dp, npad), kCapTile2, VOG_ATTN_GUARD_FLAG);
    }
    pl.add(VOG_ATTN_TILE_KERNEL, 0, g128, 256, lds, kCapLong, tile2 ? VOG_ATTN_GUARD_GATE : VOG_ATTN_GUARD_NONE);
    return 0;
  }
  if (npad <= 256) {
    // <= 8 key blocks: every operand requested in one round trip (8 waves); with out16_lo the lean form (<= 128 registers, four workgroups per CU)
    if (!a.out16_lo) pl.add(VOG_ATTN_FRAG8_KERNEL, 0, g32, 512, attn_frag8_lds(dp, npad), kCapPlain);
    else pl.add(VOG_ATTN_FRAG_LEAN_KERNEL, 0, g32, 256, attn_frag_lean_lds(npad), 0);
    return 0;
  }
  const size_t lds = attn_frag_lds(dp, npad);
  if (lds > kCapLong) VOG_FAIL(-1, "rel_attention: sequence of %d tokens exceeds the LDS budget", N);
  pl.add(VOG_ATTN_FRAG_KERNEL, 0, g32, 256, lds, kCapLong);
  return 0;
}

// vog_rel_attention_struct_fwd: first pass [, gated fallback pass]. dbg: AttnStructParams::dbg (a debug run keeps to the per-row kernels)
static int attn_struct_plan(const vog_attn_struct_args& a, int dbg, AttnPlan& pl) {
  pl.n = 0;
  if (a.dtype != VOG_BF16 && a.dtype != VOG_F16) VOG_FAIL(-1, "unknown vog_dtype %d", (int)a.dtype);
  if (!head_dim_ok(a.dp)) VOG_FAIL(-1, "struct attention: unsupported padded head dim %d (32/64/128/192/256)", a.dp);
  const int dp = a.dp, npad_kv = a.npad_kv, nsrl = a.nsrl;
  const size_t lds_row = attn_struct_row_lds(dp, npad_kv, nsrl);
  if (lds_row > kCapPlain) VOG_FAIL(-1, "struct attention: %d visual keys exceed the LDS budget", a.nppf);
  const int grid = a.S * a.H * ceil_div(ceil_div(nsrl * a.nppf, 32), 4);    // four 32-query blocks per workgroup
  const bool split = a.q_lo != nullptr;
  if (split && !(a.q_visual && a.kv_lo)) VOG_FAIL(-1, "struct attention with hi + lo operands: needs q_visual");
  if (npad_kv == 32) {
    // one visual key block. hi + lo operands: the lean form carries them (the gt5 shapes). Else, with the queries formed in the
    // kernel, every operand through LDS after one round trip; else the lean form (<= 128 registers, four workgroups per CU)
    if (split) pl.add(VOG_ATTN_STRUCT1_LEAN_KERNEL, 1, grid, 256, lds_row, 0);
    else if (a.q_visual && !a.out16_lo && nsrl <= 16 && attn_struct1_dma_lds(dp, nsrl) <= kCapDma)
      pl.add(VOG_ATTN_STRUCT1_DMA_KERNEL, 0, grid, 256, attn_struct1_dma_lds(dp, nsrl), kCapDma);
    else pl.add(VOG_ATTN_STRUCT1_LEAN_KERNEL, 0, grid, 256, lds_row, 0);
    return 0;
  }
  // several visual key blocks: K / V^T through an LDS ring shared by the workgroup (attn_struct_lds_dev.h)
  if (split) {
    // (p100) the K remainders ride in a ring of two slots. The E x F form parks 16-bit exponentials and is no candidate for
    // sharp logits: neither it nor its guard is launched.
    // (head dim 32: the 6 fragments of a key block do not divide over the 4 waves)
    if (dp < 64) VOG_FAIL(-1, "struct attention with hi + lo operands over several visual key blocks: needs a head dim of 64 / 128 / 192 / 256");
    const size_t lds = attn_struct_lds_lds(dp, npad_kv, nsrl, true);
    if (lds > kCapLong) VOG_FAIL(-1, "struct attention with hi + lo operands: %d visual keys exceed the LDS budget", a.nppf);
    pl.add(VOG_ATTN_STRUCT_LDS_KERNEL, 1, grid, 256, lds, kCapLong);
    return 0;
  }
  const size_t lds_ring = attn_struct_lds_lds(dp, npad_kv, nsrl, false);
  if (lds_ring > kCapLong) {            // the ring does not fit: per-wave loads
    pl.add(VOG_ATTN_STRUCT_KERNEL, 0, grid, 256, lds_row, 0);
    return 0;
  }
  // queries formed in the kernel, head dim 128 / 256: the E x F factorisation (attn_struct_ef_dev.h; 256 registers, two workgroups
  // per CU whose phases overlap). It needs the guard word and its fallback, the LDS-ring kernel: without them that kernel runs alone.
  const bool ef = (dp == 128 || dp == 256) && a.q_visual && npad_kv <= 512 && nsrl == EF_MAXA && !dbg && a.guard_flag;
  const size_t lds_ef = !ef ? 0 : dp == 128 ? attn_struct_ef_lds<4>(npad_kv) : attn_struct_ef_lds<8>(npad_kv);
  if (ef && lds_ef <= kCapLong) {
    pl.add(VOG_ATTN_STRUCT_EF_KERNEL, 2, a.S * a.H * ceil_div(a.nppf, 32), 256, lds_ef, kCapLong, VOG_ATTN_GUARD_FLAG);
    pl.add(VOG_ATTN_STRUCT_LDS_KERNEL, 0, grid, 256, lds_ring, kCapLong, VOG_ATTN_GUARD_GATE);
    return 0;
  }
  pl.add(VOG_ATTN_STRUCT_LDS_KERNEL, 0, grid, 256, lds_ring, kCapLong);
  return 0;
}

// Shapes the hi + lo forms cover (vog_ctx_split_supported): the hi + lo plan of the shape succeeds
int attn_split_supported(int N, int dp) {
  vog_attn_args a{};
  a.S = a.H = 1; a.N = N; a.npad = (N + 31) / 32 * 32; a.dp = dp; a.dtype = VOG_F16;
  a.q_lo = a.k_lo = &a;
  AttnPlan pl;
  return attn_plan(a, pl) == 0;
}
int attn_struct_split_supported(int nppf, int nsrl, int dp) {
  vog_attn_struct_args a{};
  a.S = a.H = 1; a.nppf = nppf; a.nsrl = nsrl; a.npad_kv = (nppf + 31) / 32 * 32; a.dp = dp; a.dtype = VOG_F16; a.q_visual = 1;
  a.q_lo = a.kv_lo = &a;
  AttnPlan pl;
  return attn_struct_plan(a, 0, pl) == 0;
}

int attn_head_pad(int dh) {
  const int opts[5] = {32, 64, 128, 192, 256};
  for (int i = 0; i < 5; ++i) if (dh <= opts[i]) return opts[i];
  return -1;
}

// ---- executor ------------------------------------------------------------------------------------------------------------------
__global__ void attn_guard_clear_kernel(int* g) { if (threadIdx.x == 0) *g = 0; }

// One launch of a plan. pa / ps: the operand block of the entry the plan came from (the other one is not read by its kernels).
// The plan's guard field decides what the kernel sees of the guard word.
template <typename T16, int NDB>
static int attn_exec(const vog_attn_launch& l, AttnParams pa, AttnStructParams ps, int* guard, hipStream_t st) {
  pa.guard = ps.guard = l.guard == VOG_ATTN_GUARD_NONE ? nullptr : guard;
  ps.guard_gate = l.guard == VOG_ATTN_GUARD_GATE;
  const dim3 grid(l.grid), block(l.block);
  const size_t cap = l.lds_cap, lds = l.lds;
  const int id = l.kernel * 4 + l.flag;      // (kernel, template flag)
  switch (id) {
    case VOG_ATTN_GUARD_CLEAR_KERNEL * 4: VOG_TRY((launch_lds<attn_guard_clear_kernel>(cap, grid, block, lds, st, guard))); break;
    case VOG_ATTN_SB_KERNEL * 4: VOG_TRY((launch_lds<attn_sb_kernel<T16, NDB, false>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_SB_KERNEL * 4 + 1: VOG_TRY((launch_lds<attn_sb_kernel<T16, NDB, true>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_FRAG_LEAN_KERNEL * 4: VOG_TRY((launch_lds<attn_frag_lean_kernel<T16, NDB, false>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_FRAG_LEAN_KERNEL * 4 + 1: VOG_TRY((launch_lds<attn_frag_lean_kernel<T16, NDB, true>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_FRAG8_KERNEL * 4: VOG_TRY((launch_lds<attn_frag8_kernel<T16, NDB>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_FRAG_KERNEL * 4: VOG_TRY((launch_lds<attn_frag_kernel<T16, NDB>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_TILE_KERNEL * 4: VOG_TRY((launch_lds<attn_tile_kernel<T16, NDB, false>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_TILE_KERNEL * 4 + 1: VOG_TRY((launch_lds<attn_tile_kernel<T16, NDB, true>>(cap, grid, block, lds, st, pa))); break;
    case VOG_ATTN_STRUCT1_LEAN_KERNEL * 4: VOG_TRY((launch_lds<attn_struct1_lean_kernel<T16, NDB, false>>(cap, grid, block, lds, st, ps))); break;
    case VOG_ATTN_STRUCT1_LEAN_KERNEL * 4 + 1: VOG_TRY((launch_lds<attn_struct1_lean_kernel<T16, NDB, true>>(cap, grid, block, lds, st, ps))); break;
    case VOG_ATTN_STRUCT1_DMA_KERNEL * 4: VOG_TRY((launch_lds<attn_struct1_dma_kernel<T16, NDB>>(cap, grid, block, lds, st, ps))); break;
    case VOG_ATTN_STRUCT_KERNEL * 4: VOG_TRY((launch_lds<attn_struct_kernel<T16, NDB>>(cap, grid, block, lds, st, ps))); break;
    case VOG_ATTN_STRUCT_LDS_KERNEL * 4: VOG_TRY((launch_lds<attn_struct_lds_kernel<T16, NDB, false>>(cap, grid, block, lds, st, ps))); break;
    default:
      // the instances that exist for some head dims only (the plans ask for no other)
      if constexpr (NDB <= 6) if (id == VOG_ATTN_TILE2_KERNEL * 4) { VOG_TRY((launch_lds<attn_tile2_kernel<T16, NDB>>(cap, grid, block, lds, st, pa))); break; }
      if constexpr (NDB >= 2) if (id == VOG_ATTN_STRUCT_LDS_KERNEL * 4 + 1) { VOG_TRY((launch_lds<attn_struct_lds_kernel<T16, NDB, true>>(cap, grid, block, lds, st, ps))); break; }
      if constexpr (NDB % 4 == 0) if (id == VOG_ATTN_STRUCT_EF_KERNEL * 4 + 2) { VOG_TRY((launch_lds<attn_struct_ef_kernel<T16, NDB, 2>>(cap, grid, block, lds, st, ps))); break; }
      VOG_FAIL(-1, "attention: no instance of %s<%d> at head dim %d", kAttnKernelNames[l.kernel], l.flag, NDB * 32);
  }
  VOG_LAUNCH_CHECK();
  return 0;
}

template <typename T16>
static int attn_exec_dp(int dp, const vog_attn_launch& l, const AttnParams& pa, const AttnStructParams& ps, int* guard, hipStream_t st) {
  switch (dp) {
    case 32: return attn_exec<T16, 1>(l, pa, ps, guard, st);
    case 64: return attn_exec<T16, 2>(l, pa, ps, guard, st);
    case 128: return attn_exec<T16, 4>(l, pa, ps, guard, st);
    case 192: return attn_exec<T16, 6>(l, pa, ps, guard, st);
    default: return attn_exec<T16, 8>(l, pa, ps, guard, st);     // (256: the plan refused every other value)
  }
}

static int attn_execute(const AttnPlan& pl, vog_dtype dtype, int dp, const AttnParams& pa, const AttnStructParams& ps, int* guard, hipStream_t st) {
  for (int i = 0; i < pl.n; ++i) VOG_DISPATCH_DTYPE(dtype, VOG_TRY(attn_exec_dp<T16>(dp, pl.l[i], pa, ps, guard, st)));
  return 0;
}

// ---- entries -------------------------------------------------------------------------------------------------------------------
static int attn_struct_dbg() {            // VOG_ATTN_STRUCT_DEBUG (perf experiments; wrong results): AttnStructParams::dbg
  static const int dbg = perf_env("VOG_ATTN_STRUCT_DEBUG") ? atoi(perf_env("VOG_ATTN_STRUCT_DEBUG")) : 0;
  return dbg;
}

int attn_struct_run(const vog_attn_struct_args* a, hipStream_t st) {
  VOG_CHECK_ARG(a && a->q && a->kv && a->vv && a->pl && a->out16);
  VOG_CHECK_ARG(a->S > 0 && a->H > 0 && a->nsrl > 0 && a->nsrl <= 32 && a->nppf > 0 && a->nfrm > 0 && a->nc_v > 0);
  VOG_CHECK_ARG((a->npad_kv % 32) == 0 && a->npad_kv >= a->nppf);
  VOG_CHECK_ARG(a->q_visual || ((a->npad_q % 32) == 0 && a->npad_q >= a->nsrl * a->nppf));
  VOG_CHECK_ARG(!a->use_rel || (a->u && a->pe_b && a->seq_per_vid > 0));
  VOG_CHECK_ARG((a->q_lo == nullptr) == (a->kv_lo == nullptr));
  AttnPlan pl;
  VOG_TRY(attn_struct_plan(*a, attn_struct_dbg(), pl));
  AttnStructParams p{(const unsigned short*)a->q, (const unsigned short*)a->kv, (const unsigned short*)a->vv, a->pl,
                     (unsigned short*)a->out16, a->u, a->pe_b, a->S, a->H, a->dp, a->nsrl, a->nppf, a->npad_q,
                     a->npad_kv, a->nfrm, a->lang_per_vid, a->nc_v, a->use_rel, a->seq_per_vid, a->NP, a->inv_scale,
                     a->q_visual ? 1 : 0, attn_struct_dbg(), nullptr, 0,
                     (const unsigned short*)a->q_lo, (const unsigned short*)a->kv_lo, (unsigned short*)a->out16_lo, a->logit_max};
  return attn_execute(pl, a->dtype, a->dp, AttnParams{}, p, a->guard_flag, st);
}

int attn_run(const vog_attn_args* a, hipStream_t st) {
  VOG_CHECK_ARG(a && a->q && a->k && a->vt && a->out16);
  VOG_CHECK_ARG(a->S > 0 && a->N > 0 && a->H > 0 && a->npad >= a->N && (a->npad % 32) == 0);
  VOG_CHECK_ARG(!a->use_rel || (a->u && a->pe_b && a->n_box > 0 && a->seq_per_vid > 0));
  VOG_CHECK_ARG((a->q_lo == nullptr) == (a->k_lo == nullptr));
  AttnPlan pl;
  VOG_TRY(attn_plan(*a, pl));
  AttnParams p{};
  p.q = (const unsigned short*)a->q; p.k = (const unsigned short*)a->k;
  p.vt = (const unsigned short*)a->vt; p.out = (unsigned short*)a->out16;
  p.u = a->u; p.pe_b = a->pe_b;
  p.S = a->S; p.N = a->N; p.H = a->H; p.dp = a->dp; p.npad = a->npad; p.use_rel = a->use_rel;
  p.n_box = a->n_box; p.seq_per_vid = a->seq_per_vid; p.NP = a->NP; p.inv_scale = a->inv_scale;
  p.guard_precleared = a->guard_precleared;
  p.q_lo = (const unsigned short*)a->q_lo; p.k_lo = (const unsigned short*)a->k_lo; p.out_lo = (unsigned short*)a->out16_lo;
  p.logit_max = a->logit_max;
  return attn_execute(pl, a->dtype, a->dp, p, AttnStructParams{}, a->guard_flag, st);
}

static int plan_out(int rc, const AttnPlan& pl, vog_attn_launch* out, int* n) {
  *n = rc == 0 ? pl.n : 0;
  for (int i = 0; i < *n; ++i) out[i] = pl.l[i];
  return rc;
}

}  // namespace vog

extern "C" int vog_rel_attention_struct_fwd(const vog_attn_struct_args* a, void* stream) {
  return vog::attn_struct_run(a, (hipStream_t)stream);
}

extern "C" int vog_rel_attention_fwd(const vog_attn_args* a, void* stream) {
  return vog::attn_run(a, (hipStream_t)stream);
}

extern "C" int vog_attn_plan(const vog_attn_args* a, vog_attn_launch* out, int* n) {
  VOG_CHECK_ARG(a && out && n);
  vog::AttnPlan pl;
  return vog::plan_out(vog::attn_plan(*a, pl), pl, out, n);
}

extern "C" int vog_attn_struct_plan(const vog_attn_struct_args* a, vog_attn_launch* out, int* n) {
  VOG_CHECK_ARG(a && out && n);
  vog::AttnPlan pl;
  return vog::plan_out(vog::attn_struct_plan(*a, vog::attn_struct_dbg(), pl), pl, out, n);
}

extern "C" const char* vog_attn_kernel_name(int kernel) {
  return kernel >= 0 && kernel < VOG_ATTN_KERNELS ? vog::kAttnKernelNames[kernel] : nullptr;
}

extern "C" int vog_attn_split_supported(int N, int dp) { return vog::attn_split_supported(N, dp); }
extern "C" int vog_attn_struct_split_supported(int nppf, int nsrl, int dp) { return vog::attn_struct_split_supported(nppf, nsrl, dp); }

