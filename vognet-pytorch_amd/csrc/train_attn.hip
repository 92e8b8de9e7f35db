// Fused attention of the training path (vog_attn_fused_f32): the semantics of vog_attn_f32 (train_tx.hip) - same inputs, same
// outputs, same dropout masks - without the [S, N, N] matrices: one forward launch and two backward launches cover all heads,
// the logits live in MFMA accumulators only, and the scratch is O(N).
//
//   logit[i, j] = (Q_h[i] . K_h[j] + relu(w_h . (box_i - box_j) + b_h)) / sqrt(d)      P = softmax_j(logit)
//   O_h = drop(P) V_h         lse[i] = log sum_j exp(logit[i, j])         delta[i] = sum_c dO[i, c] O[i, c] = sum_j P dP
//   dS = P (mask * (dO V^T) - delta) / sqrt(d)     dQ = dS K    dK = dS^T Q    dV = drop(P)^T dO
//
// A workgroup of NW waves owns 16 * NW rows of one (sequence, head) - query rows in the forward and in the dQ launch, key rows
// in the dK / dV launch - and streams the rows of the other side through LDS in sub-tiles of BS rows. A wave owns 16 of the
// rows: its operands of the products that sum over the head dimension (Q, dO | K, V) stay in registers as MFMA A fragments for
// the whole launch, its accumulators (O | dQ | dK, dV) are DP / 16 tiles of 16 x 16. The 16 x BS tile of probabilities (and of
// dS) goes through a wave-private LDS tile to become the A operand of the second product. The operand type is a template
// parameter: float on v_mfma_f32_16x16x4_f32 (exact fp32 products), bf16 / f16 on the 16x16x32 forms, where every operand is
// rounded on its way into LDS or registers (Q, K, V, dO, P, dS) and everything else stays fp32. The head dimension is padded
// with zeros to DP in LDS / registers only; tile tails use clamped row indices and masked logits.
//
// Each launch has ONE device body (fa_fwd_body, fa_bwd_q_body, fa_bwd_kv_body) that holds all of its arithmetic - logits,
// softmax, delta, dS, the bias partials, the epilogue - and is templated over a streaming policy, which alone decides how a
// sub-tile of the streamed side reaches the MFMAs: StreamPlain (attn="fused", fa_*_kernel) or StreamPipe (attn="fused_pipe",
// fa_*_pipe_kernel). The kernels are wrappers that name their LDS, build the policy and call the body - all but the plain dQ
// kernel, which keeps its statements written out (the body costs its fp32 DP 128 instance a register granule; see there).
#include <algorithm>
#include <type_traits>
#include "train_dev.h"

// The two forms of a launch must return the same bits. They share one body now, but each policy still compiles that body
// into a kernel of its own, and whether a product and a sum contract into one fused multiply-add is otherwise the optimiser's
// choice per kernel and per call site (it fused `v * inv_scale - m` for one key block of a tile and not for its neighbour). So
// the pragma stays: no fp32 statement below may contract, each rounds as it is written, in whichever kernel it is compiled.
#pragma clang fp contract(off)

namespace vog {
namespace {

constexpr int NW = 4;            // waves per workgroup
constexpr int BO = 16 * NW;      // rows a workgroup owns
constexpr float NEG = -3.0e38f;  // a masked logit

// operand type: storage in LDS, one lane's MFMA fragment, the k of one MFMA, rows per streamed tile, LDS row padding
template <typename T> struct Op;
template <> struct Op<float> {
  using St = float; using Frag = float;
  static constexpr int KC = 4, BS = 16, PAD = 4;
  static __device__ __forceinline__ St cvt(float f) { return f; }
  static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  // the lane's fragment of k0 .. k0 + KC: k contiguous at p | k strided by ld from p
  static __device__ __forceinline__ Frag ld_k(const St* p, int kg) { return p[kg]; }
  static __device__ __forceinline__ Frag ld_s(const St* p, int ld, int kg) { return p[kg * ld]; }
  // from global fp32 memory, zero from column `lim` on
  static __device__ __forceinline__ Frag ld_g(const float* p, int k0, int lim, int kg) { const int c = k0 + kg; return c < lim ? p[c] : 0.f; }
};
template <typename T16> struct Op16 {
  using St = unsigned short; using Frag = u16x8;
  static constexpr int KC = 32, BS = 32, PAD = 8;
  static __device__ __forceinline__ St cvt(float f) { return to16<T16>(f); }
  static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) { return mfma16<T16>(a, b, c); }
  static __device__ __forceinline__ Frag ld_k(const St* p, int kg) { return *(const u16x8*)(p + 8 * kg); }
  static __device__ __forceinline__ Frag ld_s(const St* p, int ld, int kg) {
    Frag f;
#pragma unroll
    for (int t = 0; t < 8; ++t) f[t] = p[(8 * kg + t) * ld];
    return f;
  }
  static __device__ __forceinline__ Frag ld_g(const float* p, int k0, int lim, int kg) {
    Frag f;
#pragma unroll
    for (int t = 0; t < 8; ++t) { const int c = k0 + 8 * kg + t; f[t] = to16<T16>(c < lim ? p[c] : 0.f); }
    return f;
  }
};
template <> struct Op<BF16> : Op16<BF16> {};
template <> struct Op<F16> : Op16<F16> {};

struct FaArgs {
  const float *q, *k, *v;          // [S*N, d] projections
  const float* dout;               // [S*N, d] gradient of the concatenated heads
  const float* cat;                // [S*N, d] the forward's output (backward)
  float* out;                      // [S*N, d] concatenated heads (forward)
  float* lse;                      // [S, H, N]
  float* delta;                    // [S, H, N]
  float *dq, *dk, *dv;             // [S*N, d]
  const float* bx;                 // [S*n, 8] normalised boxes or null
  const float *pe_w, *pe_b;        // [H, 5], [H]
  float* part;                     // [H, S * tiles, 8] bias-gradient partials or null
  int S, N, n, d, H, chunk; float inv_scale; Drop dr;
};

struct PeW { float w[5], b; };
__device__ __forceinline__ PeW load_pe(const FaArgs& a, int h) {
  PeW p{{0.f, 0.f, 0.f, 0.f, 0.f}, 0.f};
  if (a.bx) {
#pragma unroll
    for (int c = 0; c < 5; ++c) p.w[c] = a.pe_w[h * 5 + c];
    p.b = a.pe_b[h];
  }
  return p;
}
// attn_softmax_kernel's box term (train_tx.hip box_z), bi = the query's row, bj = the key's
__device__ __forceinline__ float fa_box_z(const PeW& p, const float* bi, const float* bj) {
  return p.w[0] * (bi[0] - bj[0]) + p.w[1] * (bi[1] - bj[1]) + p.w[2] * (bi[2] - bj[2]) + p.w[3] * (bi[3] - bj[3]) +
         p.w[4] * (bi[4] - bj[4]) + p.b;
}

// rows r0 .. r0 + ROWS (clamped to N - 1) of one head of x [S*N, d] into an LDS tile [ROWS][LD], columns from dh on zero
template <typename T, int DP, int ROWS>
__device__ __forceinline__ void stage_rows(typename Op<T>::St* dst, const float* x, int s, int r0, int off, int dh, const FaArgs& a, int tid) {
  constexpr int LD = DP + Op<T>::PAD;
  for (int idx = tid; idx < ROWS * DP; idx += 64 * NW) {
    const int r = idx / DP, c = idx - r * DP;
    const int row = min(r0 + r, a.N - 1);
    const float v = c < dh ? x[((int64_t)s * a.N + row) * a.d + off + c] : 0.f;
    dst[r * LD + c] = Op<T>::cvt(v);
  }
}
// the 8-float box rows of tokens r0 .. r0 + rows (clamped), indexed i % n
__device__ __forceinline__ void stage_boxes(float* dst, int s, int r0, int rows, const FaArgs& a, int tid) {
  if (!a.bx) return;
  for (int idx = tid; idx < rows * 8; idx += 64 * NW) {
    const int r = idx >> 3, c = idx & 7;
    const int row = min(r0 + r, a.N - 1);
    dst[idx] = a.bx[((int64_t)s * a.n + row % a.n) * 8 + c];
  }
}
template <typename T, int NK>
__device__ __forceinline__ void load_afrags(typename Op<T>::Frag (&f)[NK], const float* x, int s, int row, int off, int dh, const FaArgs& a, int kg) {
  const float* p = x + ((int64_t)s * a.N + min(row, a.N - 1)) * a.d + off;
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) f[kk] = Op<T>::ld_g(p, kk * Op<T>::KC, dh, kg);
}
// acc[jb] = A (registers) . B^T, B = rows jb*16 .. of an LDS tile [.][LD] (both operands contiguous in k)
template <typename T, int DP, int NJ>
__device__ __forceinline__ void mma_nt(f32x4 (&acc)[NJ], const typename Op<T>::Frag (&af)[DP / Op<T>::KC], const typename Op<T>::St* tile, int lr, int lg) {
  constexpr int LD = DP + Op<T>::PAD, KC = Op<T>::KC;
#pragma unroll
  for (int jb = 0; jb < NJ; ++jb) {
    acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < DP / KC; ++kk)
      acc[jb] = Op<T>::mma(af[kk], Op<T>::ld_k(tile + (jb * 16 + lr) * LD + kk * KC, lg), acc[jb]);
  }
}
// acc[cb] += P (wave tile [16][LDP], k contiguous) . X (LDS sub-tile [BS][LD], k = its row index), the strided operand by the
// policy's load: the same fragments into the same MFMAs in the same order under either
template <typename T, int DP, class Stream>
__device__ __forceinline__ void mma_px(f32x4 (&acc)[DP / 16], const typename Op<T>::St* ptile, const typename Op<T>::St* x, int lr, int lg) {
  constexpr int LD = DP + Op<T>::PAD, KC = Op<T>::KC, BS = Op<T>::BS, LDP = BS + Op<T>::PAD;
#pragma unroll
  for (int kk = 0; kk < BS / KC; ++kk) {
    const typename Op<T>::Frag pf = Op<T>::ld_k(ptile + lr * LDP + kk * KC, lg);
#pragma unroll
    for (int cb = 0; cb < DP / 16; ++cb)
      acc[cb] = Op<T>::mma(pf, Stream::ld_s(x + (kk * KC) * LD + cb * 16, LD, lr, lg), acc[cb]);
  }
}
__device__ __forceinline__ float red16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float red16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float red64_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct Where { int tile, s, h, off, dh; };
__device__ __forceinline__ Where where(const FaArgs& a) {
  const int nt = (a.N + BO - 1) / BO;
  Where w;
  w.tile = blockIdx.x % nt;
  const int sh = blockIdx.x / nt;
  w.h = sh % a.H; w.s = sh / a.H;
  w.off = w.h * a.chunk;
  w.dh = min(a.chunk, a.d - w.off);
  return w;
}

enum { FA_FWD, FA_BWD_Q, FA_BWD_KV };

// ---- the streaming policies ---------------------------------------------------------------------------------------------
// A policy's run<WHAT>(g0, g1, ...) walks the rows of the streamed side in ascending order and calls the body once per
// sub-tile of BS rows that starts below N, with the sub-tile as a Sub: where it starts, its two operand images [BS][LD] (g0's
// and g1's rows), its box rows and - in the dK / dV launch - its rows of lse and delta. WHAT says what a pass streams. A policy
// also supplies the ordering around the wave-private P / dS tile (ptile_reuse before the body overwrites it, ptile_ready
// before mma_px reads it) and the strided-operand load of mma_px. x0 is also the dQ body's staging room for its fp32 delta.
enum { ST_ONE, ST_TWO, ST_TWO_ROWS };    // g0 and the boxes (the forward's 16-bit lse pass) | g0, g1, boxes | and lse, delta
template <typename St> struct Sub { int j0; const St *x0, *x1; const float *bx, *lse, *delta; };

// attn="fused": ONE buffer of BS rows per operand; a barrier, stage_rows / stage_boxes, a barrier, the sub-tile. The barrier
// at the top of the loop also covers the P / dS tile's previous reads; a second one stands before mma_px.
template <typename T, int DP> struct StreamPlain {
  using St = typename Op<T>::St;
  St *x0, *x1;                 // [BS][LD] each
  float *bx, *lse, *delta;     // [BS][8]; [BS] each (ST_TWO_ROWS) or null
  template <int WHAT, class Body>
  __device__ __forceinline__ void run(const float* g0, const float* g1, const Where& at, const FaArgs& a, int tid, Body&& body) const {
    constexpr int BS = Op<T>::BS;
    for (int j0 = 0; j0 < a.N; j0 += BS) {
      __syncthreads();
      stage_rows<T, DP, BS>(x0, g0, at.s, j0, at.off, at.dh, a, tid);
      if constexpr (WHAT != ST_ONE) stage_rows<T, DP, BS>(x1, g1, at.s, j0, at.off, at.dh, a, tid);
      stage_boxes(bx, at.s, j0, BS, a, tid);
      if constexpr (WHAT == ST_TWO_ROWS) {
        if (tid < BS) {
          const int64_t o = ((int64_t)at.s * a.H + at.h) * a.N + min(j0 + tid, a.N - 1);
          lse[tid] = a.lse[o]; delta[tid] = a.delta[o];
        }
      }
      __syncthreads();
      body(Sub<St>{j0, x0, x1, bx, lse, delta});
    }
  }
  static __device__ __forceinline__ void ptile_reuse() {}
  static __device__ __forceinline__ void ptile_ready() { __syncthreads(); }
  static __device__ __forceinline__ typename Op<T>::Frag ld_s(const St* x, int ld, int lr, int lg) { return Op<T>::ld_s(x + lr, ld, lg); }
};

// attn="fused_pipe": the same sub-tiles in the same order, so the body returns the same bits. What differs:
//  - tiles of KT = NS * BS rows in TWO LDS buffers with ONE workgroup barrier per tile: while the sub-tiles of buffer b are
//    consumed in order, the rows of tile t + 1 wait in registers (fp32, as loaded; the 16-bit forms round them on their way into
//    LDS as stage_rows does) and are written to buffer b ^ 1 behind the barrier that ended tile t - 1, its last reader; the
//    loads of tile t + 2 are issued at once. The tile's box rows (and, in the dK / dV launch, its lse / delta) ride along;
//  - staging without a division: a thread owns four consecutive columns of NP rows, row and column by shifts of its index;
//    one 16-byte load per row when the head's column offset and width, the row length and the pointer allow it, else four 4-byte loads;
//    one 16- or 8-byte LDS store. Columns from dh on are zero, rows past N - 1 are clamped, as in stage_rows;
//  - no workgroup barrier around the wave-private P / dS tiles: a wave's LDS accesses execute in order, a wave-scope fence
//    keeps the compiler from moving them;
//  - the 16-bit strided operand by ds_read_b64_tr_b16, two per fragment: lane group g takes rows 8g .. 8g + 3 and 8g + 4 ..
//    8g + 7 of the k-block, lane 4q + p supplies the address of row q, columns 4p .. 4p + 3, and lane i receives column i with
//    row q in element q: f[t] = X[8g + t][col], the assignment of Op16::ld_s. Every lane supplies an in-bounds address (the
//    sub-tile loop is uniform, tiles are whole). The fp32 strided operand keeps its 4-byte reads of the padded image.
// KT: the largest of 64 | 32 rows whose four operand buffers fit 136 KB (fp32 at DP >= 192: 32, everything else: 64).
extern __shared__ __attribute__((aligned(16))) unsigned char fa_pipe_lds[];

template <typename T, int DP> struct Pipe {
  using St = typename Op<T>::St;
  static constexpr int BS = Op<T>::BS, LD = DP + Op<T>::PAD, LDP = BS + Op<T>::PAD;
  static constexpr int KT = 4 * 64 * LD * (int)sizeof(St) <= 136 * 1024 ? 64 : 32, NS = KT / BS;
  static constexpr int LC = DP <= 32 ? 3 : DP <= 64 ? 4 : DP <= 128 ? 5 : 6;     // a row is 1 << LC four-column slots (DP 192: 48 used)
  static constexpr int CPR = 1 << LC, RPP = 64 * NW / CPR, NP = KT / RPP;         // rows per pass of the workgroup, passes per tile
  static constexpr int TILE = KT * LD;                                            // one operand buffer, in St
  static_assert(KT % BS == 0 && KT % RPP == 0 && 2 * KT <= 64 * NW && CPR * 4 >= DP, "tile of whole sub-tiles, staged in whole passes");
};
template <typename T, int DP> using PipeRows = float4[Pipe<T, DP>::NP];      // a thread's share of one operand tile
template <typename T, int DP>
__device__ __forceinline__ void pipe_fetch(PipeRows<T, DP>& v, const float* x, int s, int r0, int off, int dh, const FaArgs& a, int tid) {
  using P = Pipe<T, DP>;
  const int c = (tid & (P::CPR - 1)) * 4, r = tid >> P::LC;
  if (P::CPR * 4 != DP && c >= DP) return;
  const bool vec = ((off | a.d | dh) & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;    // (precedent: frag8_f32's vec rule)
#pragma unroll
  for (int p = 0; p < P::NP; ++p) {
    const int row = min(r0 + r + p * P::RPP, a.N - 1);
    const float* src = x + ((int64_t)s * a.N + row) * a.d + off + c;
    if (vec) v[p] = c < dh ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);    // (dh % 4 == 0 here)
    else v[p] = make_float4(c < dh ? src[0] : 0.f, c + 1 < dh ? src[1] : 0.f, c + 2 < dh ? src[2] : 0.f, c + 3 < dh ? src[3] : 0.f);
  }
}
template <typename T, int DP>
__device__ __forceinline__ void pipe_park(typename Op<T>::St* dst, const PipeRows<T, DP>& v, int tid) {
  using P = Pipe<T, DP>;
  const int c = (tid & (P::CPR - 1)) * 4, r = tid >> P::LC;
  if (P::CPR * 4 != DP && c >= DP) return;
#pragma unroll
  for (int p = 0; p < P::NP; ++p) {
    typename Op<T>::St* d = dst + (r + p * P::RPP) * P::LD + c;
    if constexpr (sizeof(typename Op<T>::St) == 4) *reinterpret_cast<float4*>(d) = v[p];
    else *reinterpret_cast<u16x4*>(d) = u16x4{Op<T>::cvt(v[p].x), Op<T>::cvt(v[p].y), Op<T>::cvt(v[p].z), Op<T>::cvt(v[p].w)};
  }
}
// the box rows of tokens r0 .. r0 + KT (clamped, indexed i % n): half a row per thread
template <int KT>
__device__ __forceinline__ void pipe_fetch_boxes(float4& v, int s, int r0, const FaArgs& a, int tid) {
  if (a.bx && tid < 2 * KT) {
    const int row = min(r0 + (tid >> 1), a.N - 1);
    v = *reinterpret_cast<const float4*>(a.bx + ((int64_t)s * a.n + row % a.n) * 8 + (tid & 1) * 4);
  }
}
template <int KT>
__device__ __forceinline__ void pipe_park_boxes(float* dst, const float4& v, const FaArgs& a, int tid) {
  if (a.bx && tid < 2 * KT) *reinterpret_cast<float4*>(dst + tid * 4) = v;
}
// a wave's own LDS writes before its own LDS reads (and the reverse): nothing to wait for across waves
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Op<T>::ld_s of the k-block at x (row 0 of the block, column 0 of the 16-column group)
typedef short i16x4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ typename Op<T>::Frag pipe_ld_s(const typename Op<T>::St* x, int ld, int lr, int lg) {
  if constexpr (sizeof(typename Op<T>::St) == 4) {
    return Op<T>::ld_s(x + lr, ld, lg);
  } else {
    using LP = __attribute__((address_space(3))) i16x4*;
    const unsigned short* p = x + (8 * lg + (lr >> 2)) * ld + 4 * (lr & 3);
    const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LP)p);
    const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LP)(p + 4 * ld));
    return u16x8{(unsigned short)lo[0], (unsigned short)lo[1], (unsigned short)lo[2], (unsigned short)lo[3],
                 (unsigned short)hi[0], (unsigned short)hi[1], (unsigned short)hi[2], (unsigned short)hi[3]};
  }
}

template <typename T, int DP> struct StreamPipe {
  using St = typename Op<T>::St;
  St *x0, *x1;                 // [2][KT][LD] each
  float *bx, *lse, *delta;     // [2][KT][8]; [2][KT] each (ST_TWO_ROWS) or null
  template <int WHAT, class Body>
  __device__ __forceinline__ void run(const float* g0, const float* g1, const Where& at, const FaArgs& a, int tid, Body&& body) const {
    using P = Pipe<T, DP>;
    constexpr int BS = P::BS, LD = P::LD, KT = P::KT, NS = P::NS, TILE = P::TILE;
    const int s = at.s, off = at.off, dh = at.dh, N = a.N, nt = (N + KT - 1) / KT;
    float4 r0[P::NP], r1[P::NP], br;
    float lr_ = 0.f, dr_ = 0.f;                              // the tile's lse / delta of row tid (tid < KT)
    auto fetch = [&](int t) {
      pipe_fetch<T, DP>(r0, g0, s, t * KT, off, dh, a, tid);
      if constexpr (WHAT != ST_ONE) pipe_fetch<T, DP>(r1, g1, s, t * KT, off, dh, a, tid);
      pipe_fetch_boxes<KT>(br, s, t * KT, a, tid);
      if constexpr (WHAT == ST_TWO_ROWS) {
        if (tid < KT) {
          const int64_t o = ((int64_t)s * a.H + at.h) * N + min(t * KT + tid, N - 1);
          lr_ = a.lse[o]; dr_ = a.delta[o];
        }
      }
    };
    auto park = [&](int b) {
      pipe_park<T, DP>(x0 + b * TILE, r0, tid);
      if constexpr (WHAT != ST_ONE) pipe_park<T, DP>(x1 + b * TILE, r1, tid);
      pipe_park_boxes<KT>(bx + b * KT * 8, br, a, tid);
      if constexpr (WHAT == ST_TWO_ROWS) {
        if (tid < KT) { lse[b * KT + tid] = lr_; delta[b * KT + tid] = dr_; }
      }
    };
    fetch(0);
    park(0);
    if (nt > 1) fetch(1);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) {                     // every wave is past the barrier behind tile t - 1, the last reader of this buffer
        park((t + 1) & 1);
        if (t + 2 < nt) fetch(t + 2);
      }
      const int b = t & 1;
#pragma unroll 1
      for (int u = 0; u < NS; ++u) {
        const int j0 = t * KT + u * BS;
        if (j0 >= N) break;
        constexpr bool ROWS = WHAT == ST_TWO_ROWS;
        body(Sub<St>{j0, x0 + b * TILE + u * BS * LD, x1 + b * TILE + u * BS * LD, bx + (b * KT + u * BS) * 8,
                     ROWS ? lse + b * KT + u * BS : nullptr, ROWS ? delta + b * KT + u * BS : nullptr});
      }
      __syncthreads();
    }
  }
  static __device__ __forceinline__ void ptile_reuse() { wave_lds_order(); }
  static __device__ __forceinline__ void ptile_ready() { wave_lds_order(); }
  static __device__ __forceinline__ typename Op<T>::Frag ld_s(const St* x, int ld, int lr, int lg) { return pipe_ld_s<T>(x, ld, lr, lg); }
};

// The dynamic LDS of one pipelined launch, in bytes from fa_pipe_lds: the kernel carves from these offsets and fa_launch_dp
// asks for BYTES (the "LDS bytes" column of profiles/train_attn_pipe_kernels.md).
template <typename T, int DP, int WHICH> struct PipeLds {
  using P = Pipe<T, DP>; using St = typename P::St;
  static constexpr size_t X0 = 0;                                                  // [2][KT][LD] the first streamed operand
  static constexpr size_t X1 = X0 + 2 * P::TILE * sizeof(St);                      // [2][KT][LD] the second
  static constexpr size_t PT = X1 + 2 * P::TILE * sizeof(St);                      // [NW][16][LDP] wave tiles: P | dS | P, then dS
  static constexpr size_t BXO = PT + (WHICH == FA_BWD_KV ? 2 : 1) * NW * 16 * P::LDP * sizeof(St);   // [BO][8] the owner's boxes
  static constexpr size_t BXT = BXO + BO * 8 * 4;                                  // [2][KT][8] the tile's boxes
  static constexpr size_t E0 = BXT + 2 * P::KT * 8 * 4;                            // dQ: delta [BO] | dK / dV: lse [2][KT]
  static constexpr size_t E1 = E0 + (WHICH == FA_BWD_Q ? BO : 2 * P::KT) * 4;      // dQ: gs [NW][8] | dK / dV: delta [2][KT]
  static constexpr size_t BYTES = WHICH == FA_FWD ? E0 : E1 + (WHICH == FA_BWD_Q ? NW * 8 : 2 * P::KT) * 4;
  template <typename U> static __device__ __forceinline__ U* at(size_t o) { return reinterpret_cast<U*>(fa_pipe_lds + o); }
  static __device__ __forceinline__ StreamPipe<T, DP> stream() {
    constexpr bool ROWS = WHICH == FA_BWD_KV;
    return {at<St>(X0), at<St>(X1), at<float>(BXT), ROWS ? at<float>(E0) : nullptr, ROWS ? at<float>(E1) : nullptr};
  }
};
static_assert(PipeLds<float, 128, FA_FWD>::BYTES == 146432 && PipeLds<BF16, 32, FA_FWD>::BYTES == 31744, "the forward's table row");
static_assert(PipeLds<float, 128, FA_BWD_Q>::BYTES == 146816 && PipeLds<BF16, 32, FA_BWD_Q>::BYTES == 32128, "the dQ launch's table row");
static_assert(PipeLds<float, 128, FA_BWD_KV>::BYTES == 152576 && PipeLds<BF16, 32, FA_BWD_KV>::BYTES == 37888, "the dK / dV launch's table row");

// ---- forward: out = drop(softmax) V by online softmax, lse ---------------------------------------------------------------
// Ps [NW][16][LDP], bxo [BO][8]
template <typename T, int DP, class Stream>
__device__ __forceinline__ void fa_fwd_body(const FaArgs& a, const Stream& sm, typename Op<T>::St* Ps, float* bxo) {
  using O = Op<T>; using St = typename O::St; using Frag = typename O::Frag;
  constexpr int KC = O::KC, BS = O::BS, LDP = BS + O::PAD, NK = DP / KC, NC = DP / 16, NJ = BS / 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const Where at = where(a);
  const int s = at.s, h = at.h, off = at.off, dh = at.dh, N = a.N;
  const int i0 = at.tile * BO + w * 16;
  const bool rel = a.bx != nullptr;
  const PeW pe = load_pe(a, h);
  Frag qf[NK];
  load_afrags<T, NK>(qf, a.q, s, i0 + lr, off, dh, a, lg);
  stage_boxes(bxo, s, at.tile * BO, BO, a, tid);
  f32x4 oacc[NC];
#pragma unroll
  for (int cb = 0; cb < NC; ++cb) oacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m[4] = {NEG, NEG, NEG, NEG}, l[4] = {0.f, 0.f, 0.f, 0.f};
  St* pt = Ps + w * 16 * LDP;
  // sa = the sub-tile's scaled logits (masked past N), mx = their row maxima over this lane's columns
  auto logits = [&](const Sub<St>& t, f32x4 (&sa)[NJ], float (&mx)[4]) {
    mma_nt<T, DP, NJ>(sa, qf, t.x0, lr, lg);
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
      const int j = t.j0 + jb * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sa[jb][r];
        if (rel) v += fmaxf(fa_box_z(pe, bxo + (w * 16 + 4 * lg + r) * 8, t.bx + (jb * 16 + lr) * 8), 0.f);
        v = j < N ? v * a.inv_scale : NEG;
        sa[jb][r] = v;
        mx[r] = fmaxf(mx[r], v);
      }
    }
  };
  // 16-bit operands: autocast rounds the NORMALISED probabilities, so the row's lse is found first (a pass over the keys with
  // the logits only) and the second pass rounds exp(logit - lse); float: one pass, running maximum and sum (nothing is rounded)
  constexpr bool TWO = sizeof(St) == 2;
  if constexpr (TWO) {
    sm.template run<ST_ONE>(a.k, nullptr, at, a, tid, [&](const Sub<St>& t) {
      f32x4 sa[NJ];
      float mx[4] = {NEG, NEG, NEG, NEG};
      logits(t, sa, mx);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mn = fmaxf(m[r], red16_max(mx[r]));
        float rs = 0.f;
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) rs += t.j0 + jb * 16 + lr < N ? expf(sa[jb][r] - mn) : 0.f;
        l[r] = l[r] * expf(m[r] - mn) + red16_sum(rs);
        m[r] = mn;
      }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] += logf(l[r]); l[r] = 1.0f; }        // m := lse from here on
  }
  sm.template run<ST_TWO>(a.k, a.v, at, a, tid, [&](const Sub<St>& t) {
    f32x4 sa[NJ];
    float mx[4] = {NEG, NEG, NEG, NEG};
    logits(t, sa, mx);
    float alpha[4] = {1.f, 1.f, 1.f, 1.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!TWO) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mn = fmaxf(m[r], red16_max(mx[r]));
        alpha[r] = expf(m[r] - mn);
        m[r] = mn;
      }
    }
    Stream::ptile_reuse();                                  // the previous sub-tile's reads of pt
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
      const int j = t.j0 + jb * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * lg + r;
        float p = j < N ? expf(sa[jb][r] - m[r]) : 0.f;
        rs[r] += p;
        if (a.dr.thr) p *= drop_scale(a.dr, (((unsigned long long)s * a.H + h) * N + i) * N + j);
        pt[(4 * lg + r) * LDP + jb * 16 + lr] = O::cvt(p);
      }
    }
    if constexpr (!TWO) {
#pragma unroll
      for (int r = 0; r < 4; ++r) l[r] = l[r] * alpha[r] + red16_sum(rs[r]);
#pragma unroll
      for (int cb = 0; cb < NC; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) oacc[cb][r] *= alpha[r];
    }
    Stream::ptile_ready();
    mma_px<T, DP, Stream>(oacc, pt, t.x1, lr, lg);
  });
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * lg + r;
    if (i >= N) continue;
    const float inv = 1.0f / l[r];                         // (16-bit: 1, the probabilities were normalised)
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int c = cb * 16 + lr;
      if (c < dh) a.out[((int64_t)s * N + i) * a.d + off + c] = oacc[cb][r] * inv;
    }
    if (lr == 0) a.lse[((int64_t)s * a.H + h) * N + i] = TWO ? m[r] : m[r] + logf(l[r]);
  }
}

// ---- backward 1: per query tile - delta, dQ over the key tiles in order, the workgroup's six bias-gradient partials ---------
// Ds [NW][16][LDP], bxo [BO][8], dls [BO], gs [NW][8]. Instantiated under StreamPipe only (fa_bwd_q_kernel below says why). The
// policy comes by value here: by reference the 16-bit DP 64 pipelined instance took two more registers and with them an
// allocation granule (profiles/train_attn_onebody_kernels.md).
template <typename T, int DP, class Stream>
__device__ __forceinline__ void fa_bwd_q_body(const FaArgs& a, const Stream sm, typename Op<T>::St* Ds, float* bxo, float* dls, float (*gs)[8]) {
  using O = Op<T>; using St = typename O::St; using Frag = typename O::Frag;
  constexpr int KC = O::KC, BS = O::BS, LDP = BS + O::PAD, NK = DP / KC, NC = DP / 16, NJ = BS / 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const Where at = where(a);
  const int s = at.s, h = at.h, off = at.off, dh = at.dh, N = a.N;
  const int i0 = at.tile * BO + w * 16;
  const bool rel = a.bx != nullptr;
  const PeW pe = load_pe(a, h);
  Frag qf[NK], dof[NK];
  load_afrags<T, NK>(qf, a.q, s, i0 + lr, off, dh, a, lg);
  load_afrags<T, NK>(dof, a.dout, s, i0 + lr, off, dh, a, lg);
  stage_boxes(bxo, s, at.tile * BO, BO, a, tid);
  // delta[i] of the workgroup's rows, in fp32. float: sum_c dO[i, c] O[i, c] as the diagonal of dO O^T on the MFMA, the wave's
  // dO fragments against its 16 rows of O staged like a key tile - the summation of dP = dO V^T, so that a row with ONE key
  // (O = V) gets dP - delta = 0 exactly, as the materialised operator does. 16-bit: O was summed from ROUNDED probabilities,
  // while autocast's softmax backward sums the fp32 ones - delta = sum_j P[i, j] mask dP[i, j] in a first pass over the keys.
  float lse_r[4], dl_r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) lse_r[r] = a.lse[((int64_t)s * a.H + h) * N + min(i0 + 4 * lg + r, N - 1)];
  // the sub-tile's probabilities (0 past N), dropout factors and dP
  auto tile = [&](const Sub<St>& t, f32x4 (&pa)[NJ], f32x4 (&mk)[NJ], f32x4 (&dp)[NJ], f32x4 (&za)[NJ]) {
    mma_nt<T, DP, NJ>(pa, qf, t.x0, lr, lg);
    mma_nt<T, DP, NJ>(dp, dof, t.x1, lr, lg);
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
      const int j = t.j0 + jb * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * lg + r;
        const float z = rel ? fa_box_z(pe, bxo + (w * 16 + 4 * lg + r) * 8, t.bx + (jb * 16 + lr) * 8) : 0.f;
        const float lg_ = (pa[jb][r] + fmaxf(z, 0.f)) * a.inv_scale;
        za[jb][r] = z;
        pa[jb][r] = j < N ? expf(lg_ - lse_r[r]) : 0.f;
        mk[jb][r] = a.dr.thr ? drop_scale(a.dr, (((unsigned long long)s * a.H + h) * N + i) * N + j) : 1.0f;
      }
    }
  };
  if constexpr (sizeof(St) == 4) {                          // (four rounds per workgroup, staged by stage_rows under either policy)
    for (int ww = 0; ww < NW; ++ww) {
      __syncthreads();
      stage_rows<T, DP, 16>(sm.x0, a.cat, s, at.tile * BO + ww * 16, off, dh, a, tid);
      __syncthreads();
      if (ww != w) continue;
      f32x4 dd[1];
      mma_nt<T, DP, 1>(dd, dof, sm.x0, lr, lg);
      if ((lr >> 2) == lg) dls[w * 16 + lr] = (lr & 3) == 0 ? dd[0][0] : (lr & 3) == 1 ? dd[0][1] : (lr & 3) == 2 ? dd[0][2] : dd[0][3];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) dl_r[r] = dls[w * 16 + 4 * lg + r];
  } else {
    sm.template run<ST_TWO>(a.k, a.v, at, a, tid, [&](const Sub<St>& t) {
      f32x4 pa[NJ], mk[NJ], dp[NJ], za[NJ];
      tile(t, pa, mk, dp, za);
#pragma unroll
      for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dl_r[r] += pa[jb][r] * (mk[jb][r] * dp[jb][r]);
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) dl_r[r] = red16_sum(dl_r[r]);
  }
  if (lr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i0 + 4 * lg + r < N) a.delta[((int64_t)s * a.H + h) * N + i0 + 4 * lg + r] = dl_r[r];
  }
  f32x4 dqacc[NC];
#pragma unroll
  for (int cb = 0; cb < NC; ++cb) dqacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  St* dt = Ds + w * 16 * LDP;
  sm.template run<ST_TWO>(a.k, a.v, at, a, tid, [&](const Sub<St>& t) {
    f32x4 pa[NJ], mk[NJ], dp[NJ], za[NJ];
    tile(t, pa, mk, dp, za);
    Stream::ptile_reuse();                                  // the previous sub-tile's reads of dt
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * lg + r;
        const float* bi = bxo + (w * 16 + 4 * lg + r) * 8;
        const float* bj = t.bx + (jb * 16 + lr) * 8;
        const float ds = pa[jb][r] * (mk[jb][r] * dp[jb][r] - dl_r[r]) * a.inv_scale;
        dt[(4 * lg + r) * LDP + jb * 16 + lr] = O::cvt(ds);
        if (rel && za[jb][r] > 0.f && i < N) {
#pragma unroll
          for (int c = 0; c < 5; ++c) g[c] += ds * (bi[c] - bj[c]);
          g[5] += ds;
        }
      }
    }
    Stream::ptile_ready();
    mma_px<T, DP, Stream>(dqacc, dt, t.x0, lr, lg);
  });
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * lg + r;
    if (i >= N) continue;
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int c = cb * 16 + lr;
      if (c < dh) a.dq[((int64_t)s * N + i) * a.d + off + c] = dqacc[cb][r];
    }
  }
  if (a.part) {                                            // fixed order: lanes (butterfly), then the waves 0 .. NW - 1
#pragma unroll
    for (int c = 0; c < 6; ++c) g[c] = red64_sum(g[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) gs[w][c] = g[c];
      gs[w][6] = gs[w][7] = 0.f;
    }
    __syncthreads();
    if (tid < 8) {
      float t = 0.f;
      for (int ww = 0; ww < NW; ++ww) t += gs[ww][tid];
      const int nt = (N + BO - 1) / BO;
      a.part[(((int64_t)h * a.S + s) * nt + at.tile) * 8 + tid] = t;
    }
  }
}

// ---- backward 2: per key tile - dK = dS^T Q and dV = drop(P)^T dO over the query tiles in order ------------------------------
// The products are formed transposed: S^T = K Q^T and dP^T = V dO^T have the key on the accumulator's row, the wave's own.
// Pt, Dt [NW][16][LDP] each, bxo [BO][8]
template <typename T, int DP, class Stream>
__device__ __forceinline__ void fa_bwd_kv_body(const FaArgs& a, const Stream& sm, typename Op<T>::St* Pt, typename Op<T>::St* Dt, float* bxo) {
  using O = Op<T>; using St = typename O::St; using Frag = typename O::Frag;
  constexpr int KC = O::KC, BS = O::BS, LDP = BS + O::PAD, NK = DP / KC, NC = DP / 16, NJ = BS / 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const Where at = where(a);
  const int s = at.s, h = at.h, off = at.off, dh = at.dh, N = a.N;
  const int jw = at.tile * BO + w * 16;
  const bool rel = a.bx != nullptr;
  const PeW pe = load_pe(a, h);
  Frag kf[NK], vf[NK];
  load_afrags<T, NK>(kf, a.k, s, jw + lr, off, dh, a, lg);
  load_afrags<T, NK>(vf, a.v, s, jw + lr, off, dh, a, lg);
  stage_boxes(bxo, s, at.tile * BO, BO, a, tid);
  f32x4 dkacc[NC], dvacc[NC];
#pragma unroll
  for (int cb = 0; cb < NC; ++cb) { dkacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; dvacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  St* pt = Pt + w * 16 * LDP;
  St* dt = Dt + w * 16 * LDP;
  sm.template run<ST_TWO_ROWS>(a.q, a.dout, at, a, tid, [&](const Sub<St>& t) {
    const int i0 = t.j0;
    f32x4 sa[NJ], dp[NJ];
    mma_nt<T, DP, NJ>(sa, kf, t.x0, lr, lg);
    mma_nt<T, DP, NJ>(dp, vf, t.x1, lr, lg);
    Stream::ptile_reuse();                                  // the previous sub-tile's reads of pt / dt
#pragma unroll
    for (int ib = 0; ib < NJ; ++ib) {
      const int il = ib * 16 + lr, i = i0 + il;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jw + 4 * lg + r;
        const float z = rel ? fa_box_z(pe, t.bx + il * 8, bxo + (w * 16 + 4 * lg + r) * 8) : 0.f;
        const float lg_ = (sa[ib][r] + fmaxf(z, 0.f)) * a.inv_scale;
        const float p = i < N ? expf(lg_ - t.lse[il]) : 0.f;
        const float mk = a.dr.thr ? drop_scale(a.dr, (((unsigned long long)s * a.H + h) * N + i) * N + j) : 1.0f;
        const float ds = p * (mk * dp[ib][r] - t.delta[il]) * a.inv_scale;
        pt[(4 * lg + r) * LDP + il] = O::cvt(p * mk);
        dt[(4 * lg + r) * LDP + il] = O::cvt(ds);
      }
    }
    Stream::ptile_ready();
    mma_px<T, DP, Stream>(dvacc, pt, t.x1, lr, lg);
    mma_px<T, DP, Stream>(dkacc, dt, t.x0, lr, lg);
  });
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = jw + 4 * lg + r;
    if (j >= N) continue;
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int c = cb * 16 + lr;
      if (c < dh) {
        const int64_t o = ((int64_t)s * N + j) * a.d + off + c;
        a.dk[o] = dkacc[cb][r]; a.dv[o] = dvacc[cb][r];
      }
    }
  }
}

// ---- the six kernels: the LDS of the form, its policy, the body (the plain dQ kernel: written out) ---------------------------
template <typename T, int DP>
__global__ __launch_bounds__(64 * NW) void fa_fwd_kernel(FaArgs a) {
  using St = typename Op<T>::St;
  constexpr int BS = Op<T>::BS, LD = DP + Op<T>::PAD, LDP = BS + Op<T>::PAD;
  __shared__ __attribute__((aligned(16))) St Ks[BS * LD];
  __shared__ __attribute__((aligned(16))) St Vs[BS * LD];
  __shared__ __attribute__((aligned(16))) St Ps[NW * 16 * LDP];
  __shared__ float bxo[BO * 8], bxs[BS * 8];
  fa_fwd_body<T, DP>(a, StreamPlain<T, DP>{Ks, Vs, bxs, nullptr, nullptr}, Ps, bxo);
}
// The plain dQ launch is NOT fa_bwd_q_body under StreamPlain (it compiles and returns the same bits): through the body every
// plain fp32 instance keeps two more architectural registers, which costs fa_bwd_q_kernel<float, 128> an allocation granule
// (159 + 40 -> 161 + 40, 200 -> 208 allocated; profiles/train_attn_onebody_kernels.md). So this kernel keeps the statements of
// fa_bwd_q_body written out with its staging inside `tile`; a change to the arithmetic of the dQ launch is made in both, and
// tests/test_gpu_train_attn_pipe.py holds the two to the same bits.
template <typename T, int DP>
__global__ __launch_bounds__(64 * NW) void fa_bwd_q_kernel(FaArgs a) {
  using O = Op<T>; using St = typename O::St; using Frag = typename O::Frag;
  constexpr int KC = O::KC, BS = O::BS, LD = DP + O::PAD, LDP = BS + O::PAD, NK = DP / KC, NC = DP / 16, NJ = BS / 16;
  __shared__ __attribute__((aligned(16))) St Ks[BS * LD];
  __shared__ __attribute__((aligned(16))) St Vs[BS * LD];
  __shared__ __attribute__((aligned(16))) St Ds[NW * 16 * LDP];
  __shared__ float bxo[BO * 8], bxs[BS * 8], dls[BO], gs[NW][8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const Where at = where(a);
  const int s = at.s, h = at.h, off = at.off, dh = at.dh, N = a.N;
  const int i0 = at.tile * BO + w * 16;
  const bool rel = a.bx != nullptr;
  const PeW pe = load_pe(a, h);
  Frag qf[NK], dof[NK];
  load_afrags<T, NK>(qf, a.q, s, i0 + lr, off, dh, a, lg);
  load_afrags<T, NK>(dof, a.dout, s, i0 + lr, off, dh, a, lg);
  stage_boxes(bxo, s, at.tile * BO, BO, a, tid);
  float lse_r[4], dl_r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) lse_r[r] = a.lse[((int64_t)s * a.H + h) * N + min(i0 + 4 * lg + r, N - 1)];
  // the tile's probabilities (0 past N), dropout factors and dP
  auto tile = [&](int j0, f32x4 (&pa)[NJ], f32x4 (&mk)[NJ], f32x4 (&dp)[NJ], f32x4 (&za)[NJ]) {
    __syncthreads();
    stage_rows<T, DP, BS>(Ks, a.k, s, j0, off, dh, a, tid);
    stage_rows<T, DP, BS>(Vs, a.v, s, j0, off, dh, a, tid);
    stage_boxes(bxs, s, j0, BS, a, tid);
    __syncthreads();
    mma_nt<T, DP, NJ>(pa, qf, Ks, lr, lg);
    mma_nt<T, DP, NJ>(dp, dof, Vs, lr, lg);
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
      const int j = j0 + jb * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * lg + r;
        const float z = rel ? fa_box_z(pe, bxo + (w * 16 + 4 * lg + r) * 8, bxs + (jb * 16 + lr) * 8) : 0.f;
        const float lg_ = (pa[jb][r] + fmaxf(z, 0.f)) * a.inv_scale;
        za[jb][r] = z;
        pa[jb][r] = j < N ? expf(lg_ - lse_r[r]) : 0.f;
        mk[jb][r] = a.dr.thr ? drop_scale(a.dr, (((unsigned long long)s * a.H + h) * N + i) * N + j) : 1.0f;
      }
    }
  };
  if constexpr (sizeof(St) == 4) {
    for (int ww = 0; ww < NW; ++ww) {
      __syncthreads();
      stage_rows<T, DP, 16>(Ks, a.cat, s, at.tile * BO + ww * 16, off, dh, a, tid);
      __syncthreads();
      if (ww != w) continue;
      f32x4 dd[1];
      mma_nt<T, DP, 1>(dd, dof, Ks, lr, lg);
      if ((lr >> 2) == lg) dls[w * 16 + lr] = (lr & 3) == 0 ? dd[0][0] : (lr & 3) == 1 ? dd[0][1] : (lr & 3) == 2 ? dd[0][2] : dd[0][3];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) dl_r[r] = dls[w * 16 + 4 * lg + r];
  } else {
    for (int j0 = 0; j0 < N; j0 += BS) {
      f32x4 pa[NJ], mk[NJ], dp[NJ], za[NJ];
      tile(j0, pa, mk, dp, za);
#pragma unroll
      for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) dl_r[r] += pa[jb][r] * (mk[jb][r] * dp[jb][r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dl_r[r] = red16_sum(dl_r[r]);
  }
  if (lr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i0 + 4 * lg + r < N) a.delta[((int64_t)s * a.H + h) * N + i0 + 4 * lg + r] = dl_r[r];
  }
  f32x4 dqacc[NC];
#pragma unroll
  for (int cb = 0; cb < NC; ++cb) dqacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  St* dt = Ds + w * 16 * LDP;
  for (int j0 = 0; j0 < N; j0 += BS) {
    f32x4 pa[NJ], mk[NJ], dp[NJ], za[NJ];
    tile(j0, pa, mk, dp, za);
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * lg + r;
        const float* bi = bxo + (w * 16 + 4 * lg + r) * 8;
        const float* bj = bxs + (jb * 16 + lr) * 8;
        const float ds = pa[jb][r] * (mk[jb][r] * dp[jb][r] - dl_r[r]) * a.inv_scale;
        dt[(4 * lg + r) * LDP + jb * 16 + lr] = O::cvt(ds);
        if (rel && za[jb][r] > 0.f && i < N) {
#pragma unroll
          for (int c = 0; c < 5; ++c) g[c] += ds * (bi[c] - bj[c]);
          g[5] += ds;
        }
      }
    }
    __syncthreads();
    mma_px<T, DP, StreamPlain<T, DP>>(dqacc, dt, Ks, lr, lg);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * lg + r;
    if (i >= N) continue;
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
      const int c = cb * 16 + lr;
      if (c < dh) a.dq[((int64_t)s * N + i) * a.d + off + c] = dqacc[cb][r];
    }
  }
  if (a.part) {                                            // fixed order: lanes (butterfly), then the waves 0 .. NW - 1
#pragma unroll
    for (int c = 0; c < 6; ++c) g[c] = red64_sum(g[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) gs[w][c] = g[c];
      gs[w][6] = gs[w][7] = 0.f;
    }
    __syncthreads();
    if (tid < 8) {
      float t = 0.f;
      for (int ww = 0; ww < NW; ++ww) t += gs[ww][tid];
      const int nt = (N + BO - 1) / BO;
      a.part[(((int64_t)h * a.S + s) * nt + at.tile) * 8 + tid] = t;
    }
  }
}
template <typename T, int DP>
__global__ __launch_bounds__(64 * NW) void fa_bwd_kv_kernel(FaArgs a) {
  using St = typename Op<T>::St;
  constexpr int BS = Op<T>::BS, LD = DP + Op<T>::PAD, LDP = BS + Op<T>::PAD;
  __shared__ __attribute__((aligned(16))) St Qs[BS * LD];
  __shared__ __attribute__((aligned(16))) St Os[BS * LD];
  __shared__ __attribute__((aligned(16))) St Pt[NW * 16 * LDP];
  __shared__ __attribute__((aligned(16))) St Dt[NW * 16 * LDP];
  __shared__ float bxo[BO * 8], bxs[BS * 8], lses[BS], dls[BS];
  fa_bwd_kv_body<T, DP>(a, StreamPlain<T, DP>{Qs, Os, bxs, lses, dls}, Pt, Dt, bxo);
}
template <typename T, int DP>
__global__ __launch_bounds__(64 * NW) void fa_fwd_pipe_kernel(FaArgs a) {
  using Y = PipeLds<T, DP, FA_FWD>; using St = typename Y::St;
  fa_fwd_body<T, DP>(a, Y::stream(), Y::template at<St>(Y::PT), Y::template at<float>(Y::BXO));
}
template <typename T, int DP>
__global__ __launch_bounds__(64 * NW) void fa_bwd_q_pipe_kernel(FaArgs a) {
  using Y = PipeLds<T, DP, FA_BWD_Q>; using St = typename Y::St;
  fa_bwd_q_body<T, DP>(a, Y::stream(), Y::template at<St>(Y::PT), Y::template at<float>(Y::BXO), Y::template at<float>(Y::E0),
                       Y::template at<float[8]>(Y::E1));
}
template <typename T, int DP>
__global__ __launch_bounds__(64 * NW) void fa_bwd_kv_pipe_kernel(FaArgs a) {
  using Y = PipeLds<T, DP, FA_BWD_KV>; using St = typename Y::St;
  fa_bwd_kv_body<T, DP>(a, Y::stream(), Y::template at<St>(Y::PT), Y::template at<St>(Y::PT) + NW * 16 * Y::P::LDP,
                        Y::template at<float>(Y::BXO));
}

// g_pe_w[h, :] / g_pe_b[h] = the sum of head h's partials in a fixed order: 8 strided runs, then the runs 0 .. 7
__global__ __launch_bounds__(64) void fa_pe_sum_kernel(const float* part, float* g_w, float* g_b, int cnt) {
  __shared__ float red[8][8];
  const int h = blockIdx.x, c = threadIdx.x & 7, grp = threadIdx.x >> 3;
  float t = 0.f;
  for (int k = grp; k < cnt; k += 8) t += part[((int64_t)h * cnt + k) * 8 + c];
  red[grp][c] = t;
  __syncthreads();
  if (threadIdx.x < 6) {
    float u = 0.f;
    for (int q = 0; q < 8; ++q) u += red[q][threadIdx.x];
    if (threadIdx.x < 5) g_w[h * 5 + threadIdx.x] = u; else g_b[h] = u;
  }
}

template <typename T, int DP>
int fa_launch_dp(int which, dim3 grid, hipStream_t st, const FaArgs& a) {
  if (train_int(TRAIN_ATTN_FUSED_PIPE)) {                  // the pipelined forms: dynamic LDS above the 64 KB a kernel gets unasked
    constexpr size_t fwd = PipeLds<T, DP, FA_FWD>::BYTES, bq = PipeLds<T, DP, FA_BWD_Q>::BYTES, bkv = PipeLds<T, DP, FA_BWD_KV>::BYTES;
    static_assert(fwd <= 156 * 1024 && bq <= 156 * 1024 && bkv <= 156 * 1024, "a workgroup's LDS");
    if (which == FA_FWD) VOG_TRY((launch_lds<fa_fwd_pipe_kernel<T, DP>>(fwd, grid, dim3(64 * NW), fwd, st, a)));
    else if (which == FA_BWD_Q) VOG_TRY((launch_lds<fa_bwd_q_pipe_kernel<T, DP>>(bq, grid, dim3(64 * NW), bq, st, a)));
    else VOG_TRY((launch_lds<fa_bwd_kv_pipe_kernel<T, DP>>(bkv, grid, dim3(64 * NW), bkv, st, a)));
    ++train_int(TRAIN_ATTN_FUSED_PIPE_LAUNCHES);
    return 0;
  }
  if (which == FA_FWD) ::vog::launch(fa_fwd_kernel<T, DP>, grid, dim3(64 * NW), 0, st, a);
  else if (which == FA_BWD_Q) ::vog::launch(fa_bwd_q_kernel<T, DP>, grid, dim3(64 * NW), 0, st, a);
  else ::vog::launch(fa_bwd_kv_kernel<T, DP>, grid, dim3(64 * NW), 0, st, a);
  return 0;
}
// DP: the head size rounded up to an instantiated multiple of 32 (the k of the 16-bit MFMA)
template <typename T>
int fa_launch(int which, int dp, dim3 grid, hipStream_t st, const FaArgs& a) {
  if (dp <= 32) return fa_launch_dp<T, 32>(which, grid, st, a);
  if (dp <= 64) return fa_launch_dp<T, 64>(which, grid, st, a);
  if (dp <= 128) return fa_launch_dp<T, 128>(which, grid, st, a);
  if (dp <= 192) return fa_launch_dp<T, 192>(which, grid, st, a);
  return fa_launch_dp<T, 256>(which, grid, st, a);
}
int fa_launch_amp(int amp, int which, int dp, dim3 grid, hipStream_t st, const FaArgs& a) {
  if (amp == 0) { VOG_TRY(fa_launch<float>(which, dp, grid, st, a)); count_f32_product(); return 0; }
  if (amp == 1) return fa_launch<BF16>(which, dp, grid, st, a);
  return fa_launch<F16>(which, dp, grid, st, a);
}

struct FusedBufs { float *q, *k, *v, *dq, *dk, *dv, *bx, *delta, *lse, *cat, *part; int64_t bytes; };
FusedBufs fused_layout(void* base, int S, int N, int n, int d, int H) {
  Carve c(base, 4, true);
  FusedBufs b;
  const int64_t M = (int64_t)S * N;
  for (float** p : {&b.q, &b.k, &b.v, &b.dq, &b.dk, &b.dv}) *p = c.take<float>(M * d);
  b.bx = c.take<float>((int64_t)S * n * 8);                            // normalised boxes
  b.delta = c.take<float>(M * H);                                      // [S, H, N]
  b.lse = c.take<float>(M * H);                                        // the recompute form's own lse / cat
  b.cat = c.take<float>(M * d);
  b.part = c.take<float>((int64_t)H * S * ((N + BO - 1) / BO) * 8);    // one row of bias-gradient partials per dQ workgroup
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace vog

using namespace vog;

extern "C" int64_t vog_attn_fused_scratch_bytes(int S, int N, int n, int d, int n_heads) {
  if (S <= 0 || N <= 0 || n <= 0 || d <= 0 || n_heads <= 0) return -1;
  return fused_layout(nullptr, S, N, n, d, n_heads).bytes;
}

// vl (vog_attn_fused_f32_vl): the input as its factors - q, k, v come from vl_forward, the gradients behind dq, dk, dv from
// vl_backward (train_tx.hip)
static int attn_fused_body(const vog_attn_fused_args* a, const vog_attn_vl* vl, void* stream) {
  VOG_CHECK_ARG(a && (vl || a->x) && a->wq && a->wk && a->wv && a->scratch && a->S > 0 && a->N > 0 && a->n > 0 && a->d > 0 && a->n_heads > 0);
  VOG_CHECK_ARG((a->N % a->n) == 0 && a->n_heads <= a->d);
  const bool bwd = a->d_cat != nullptr, rel = a->props != nullptr, kept = bwd && a->kept_forward;
  if (rel) VOG_CHECK_ARG(a->pe_w && a->pe_b && a->prop_stride >= 5 && a->vid_w > 0.f && a->vid_h > 0.f && a->nfrm_div > 0.f);
  if (bwd && rel) VOG_CHECK_ARG(!a->g_pe_w == !a->g_pe_b);
  if (!bwd) VOG_CHECK_ARG(a->cat_out);
  if (kept) VOG_CHECK_ARG(a->lse && a->cat && !a->cat_out);               // the forward of this very input: nothing to recompute
  const int S = a->S, N = a->N, n = a->n, d = a->d, H = a->n_heads, M = S * N;
  const int chunk = (d + H - 1) / H;                                     // torch.chunk split sizes (transformer_code.py:66-67)
  if (d - (H - 1) * chunk <= 0) VOG_FAIL(-1, "vog_attn_fused_f32: %d heads do not split %d features", H, d);
  if (chunk > 256) VOG_FAIL(-1, "vog_attn_fused_f32: head size %d above 256", chunk);
  if (vl) VOG_TRY(vl_check(vl, a->d_x, S, N, n, d));
  const int nt = ceil_div(N, BO);
  VOG_CHECK_ARG((int64_t)S * H * nt < (int64_t)1 << 31);
  if ((int64_t)a->scratch_bytes < vog_attn_fused_scratch_bytes(S, N, n, d, H)) VOG_FAIL(-2, "vog_attn_fused_f32: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const FusedBufs b = fused_layout(a->scratch, S, N, n, d, H);
  const bool any_dx = a->d_x || (vl && (vl->d_ps || vl->d_lang));
  const bool need_dq = a->g_wq || any_dx, need_dk = a->g_wk || any_dx, need_dv = a->g_wv || any_dx;
  const bool pe_grad = bwd && rel && a->g_pe_w;
  // q, k, v = x W^T  (transformer_code.py:136-150; no bias): train_gemm.hip's products, under the thread's amp / bf16_gemm switches
  if (vl) {
    VOG_TRY(vl_forward(vl, a->wq, a->wk, a->wv, b.q, b.k, b.v, n, st));
  } else {
    VOG_TRY(gemm_f32(a->x, d, 1, a->wq, 1, d, b.q, d, nullptr, 0, M, d, d, st));
    VOG_TRY(gemm_f32(a->x, d, 1, a->wk, 1, d, b.k, d, nullptr, 0, M, d, d, st));
    VOG_TRY(gemm_f32(a->x, d, 1, a->wv, 1, d, b.v, d, nullptr, 0, M, d, d, st));
  }
  if (rel)
    norm_boxes(a->props, a->prop_stride, a->vid_w, a->vid_h, a->nfrm_div, b.bx, S * n, st);
  FaArgs f{};
  f.q = b.q; f.k = b.k; f.v = b.v; f.dq = b.dq; f.dk = b.dk; f.dv = b.dv; f.delta = b.delta;
  f.bx = rel ? b.bx : nullptr; f.pe_w = a->pe_w; f.pe_b = a->pe_b;
  f.S = S; f.N = N; f.n = n; f.d = d; f.H = H; f.chunk = chunk;
  f.inv_scale = 1.0f / sqrtf((float)d);                                  // scale = sqrt(d_model)
  f.dr = make_drop(a->drop_p, a->drop_seed, a->drop_site);
  const int amp = train_amp(), dp = (chunk + 31) / 32 * 32;
  const dim3 grid((unsigned)(S * H * nt));
  if (!kept) {                                                           // the forward, also what the stand-alone backward starts from
    f.out = a->cat_out ? a->cat_out : b.cat;
    f.lse = a->lse ? a->lse : b.lse;
    VOG_TRY(fa_launch_amp(amp, FA_FWD, dp, grid, st, f));
    f.cat = f.out;
  } else {
    f.cat = a->cat; f.lse = a->lse;
  }
  if (bwd && (need_dq || need_dk || need_dv || pe_grad)) {
    f.dout = a->d_cat;
    f.part = pe_grad ? b.part : nullptr;
    VOG_TRY(fa_launch_amp(amp, FA_BWD_Q, dp, grid, st, f));              // delta, dQ, the bias partials
    if (need_dk || need_dv) VOG_TRY(fa_launch_amp(amp, FA_BWD_KV, dp, grid, st, f));
    if (pe_grad) ::vog::launch(fa_pe_sum_kernel, dim3(H), dim3(64), 0, st, (const float*)b.part, a->g_pe_w, a->g_pe_b, S * nt);
    if (vl) VOG_TRY(vl_backward(vl, a->wq, a->wk, a->wv, b.dq, b.dk, b.dv, a->g_wq, a->g_wk, a->g_wv, n, st));
    if (!vl && a->g_wq) VOG_TRY(gemm_f32(b.dq, 1, d, a->x, d, 1, a->g_wq, d, nullptr, 0, d, d, M, st));      // d Wq = dQ^T x
    if (!vl && a->g_wk) VOG_TRY(gemm_f32(b.dk, 1, d, a->x, d, 1, a->g_wk, d, nullptr, 0, d, d, M, st));
    if (!vl && a->g_wv) VOG_TRY(gemm_f32(b.dv, 1, d, a->x, d, 1, a->g_wv, d, nullptr, 0, d, d, M, st));
    if (a->d_x) {
      VOG_TRY(gemm_f32(b.dq, d, 1, a->wq, d, 1, a->d_x, d, nullptr, 0, M, d, d, st, a->accumulate_dx ? 1 : 0));   // dx (+)= dQ Wq + dK Wk + dV Wv
      VOG_TRY(gemm_f32(b.dk, d, 1, a->wk, d, 1, a->d_x, d, nullptr, 0, M, d, d, st, 1));
      VOG_TRY(gemm_f32(b.dv, d, 1, a->wv, d, 1, a->d_x, d, nullptr, 0, M, d, d, st, 1));
    }
  }
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_attn_fused_f32(const vog_attn_fused_args* a, void* stream) { return attn_fused_body(a, nullptr, stream); }

extern "C" int vog_attn_fused_f32_vl(const vog_attn_fused_args* a, const vog_attn_vl* vl, void* stream) {
  VOG_CHECK_ARG(vl);
  return attn_fused_body(a, vl, stream);
}
