// The products of the fp32 / mixed-precision training path: the 128 x 64 tile GEMM on the fp32 and on the 16-bit matrix pipe,
// the pipelined 16-bit tile GEMM, the weight-stream kernel of the BiLSTM's recurrent products, split-K, the transpose, and the
// calling thread's precision switches (vog_train_set_int / vog_train_get_int).
#include <map>
#include <mutex>
#include <type_traits>
#include "train_dev.h"

namespace vog {

// ---- C[M,N] = A . B (+ bias[n]) (relu), generic strides: A(m,k) = a[m*am + k*ak], B(k,n) = b[k*bk + n*bn] --------
// One of (am, ak) and one of (bk, bn) is 1 (row- or column-major operands; the launcher checks it), every
// dimension is a multiple of 4 and the pointers are 16-byte aligned: tiles are fetched with 16-byte loads
// along the unit stride, one chunk ahead of the MFMAs (registers), and parked in LDS as [k][m] / [k][n].
// 128 x 64 tile per workgroup, 4 waves of 64 x 32 (4 x 2 MFMA tiles of 16 x 16), K in chunks of 16.
struct GemmF32 {
  const float* a; int64_t am, ak; const float* b; int64_t bk, bn; float* c; int64_t ldc;
  const float* bias; int relu; int M, N, K;
  int64_t sa, sb, sc;       // batch strides (blockIdx.z)
  int accum;                // C += ...
  int scalar;               // any dimensions / alignments: element loads with per-element bounds checks
  int kchunk;               // split K: block z handles k in [z * kchunk, ...) (sa / sb advance a / b by a chunk, sc = one partial C)
};

// What the tile kernels below share. Prologue: this block's operands and output (batch or split-K chunk blockIdx.z) and the
// length KL of its K range. Epilogue: a wave's MI x NJ MFMA tiles (+ bias, relu, accumulate) from (m0, n0) on.
struct GemmBatch { const float *pa, *pb; float* pc; int KL; };
__device__ __forceinline__ GemmBatch gemm_tile_batch(const GemmF32& p) {
  GemmBatch z{p.a + (int64_t)blockIdx.z * p.sa, p.b + (int64_t)blockIdx.z * p.sb, p.c + (int64_t)blockIdx.z * p.sc, p.K};
  if (p.kchunk) z.KL = p.K - (int)blockIdx.z * p.kchunk < p.kchunk ? p.K - (int)blockIdx.z * p.kchunk : p.kchunk;
  return z;
}
template <int MI, int NJ>
__device__ __forceinline__ void gemm_tile_store(const GemmF32& p, float* pc, const f32x4 (&acc)[MI][NJ], int m0, int n0, int lane) {
  // D: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + i * 16 + (lane >> 4) * 4 + r, n = n0 + j * 16 + (lane & 15);
        if (m < p.M && n < p.N) {
          float v = acc[i][j][r];
          if (p.bias) v += p.bias[n];
          if (p.relu) v = v < 0.f ? 0.f : v;
          float* dst = pc + (int64_t)m * p.ldc + n;
          *dst = p.accum ? *dst + v : v;
        }
      }
}

__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmF32 p) {
  constexpr int TM = 128, TN = 64, TK = 16;
  __shared__ __attribute__((aligned(16))) float As[TK][TM + 4];      // [k][m]
  __shared__ __attribute__((aligned(16))) float Bs[TK][TN + 4];      // [k][n]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 32;
  const GemmBatch z = gemm_tile_batch(p);
  const float *pa = z.pa, *pb = z.pb; float* pc = z.pc; const int KL = z.KL;
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool a_kfast = p.ak == 1, b_nfast = p.bn == 1;
  float4 ra[2], rb;
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int idx = tid + e * 256;
      int m, k;
      if (a_kfast) { m = idx >> 2; k = (idx & 3) * 4; } else { k = idx >> 5; m = (idx & 31) * 4; }
      const int gm = m0 + m, gk = k0 + k;
      if (!p.scalar) {
        ra[e] = (gm < p.M && gk < KL) ? *reinterpret_cast<const float4*>(pa + (int64_t)gm * p.am + (int64_t)gk * p.ak)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int mm = a_kfast ? gm : gm + q, kk = a_kfast ? gk + q : gk;
          v[q] = (mm < p.M && kk < KL) ? pa[(int64_t)mm * p.am + (int64_t)kk * p.ak] : 0.f;
        }
        ra[e] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    int n, k;
    if (b_nfast) { k = tid >> 4; n = (tid & 15) * 4; } else { n = tid >> 2; k = (tid & 3) * 4; }
    const int gn = n0 + n, gk = k0 + k;
    if (!p.scalar) {
      rb = (gn < p.N && gk < KL) ? *reinterpret_cast<const float4*>(pb + (int64_t)gk * p.bk + (int64_t)gn * p.bn)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nn = b_nfast ? gn + q : gn, kk = b_nfast ? gk : gk + q;
        v[q] = (nn < p.N && kk < KL) ? pb[(int64_t)kk * p.bk + (int64_t)nn * p.bn] : 0.f;
      }
      rb = make_float4(v[0], v[1], v[2], v[3]);
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int idx = tid + e * 256;
      if (a_kfast) {
        const int m = idx >> 2, k = (idx & 3) * 4;
        As[k][m] = ra[e].x; As[k + 1][m] = ra[e].y; As[k + 2][m] = ra[e].z; As[k + 3][m] = ra[e].w;
      } else {
        const int k = idx >> 5, m = (idx & 31) * 4;
        *reinterpret_cast<float4*>(&As[k][m]) = ra[e];
      }
    }
    if (b_nfast) {
      const int k = tid >> 4, n = (tid & 15) * 4;
      *reinterpret_cast<float4*>(&Bs[k][n]) = rb;
    } else {
      const int n = tid >> 2, k = (tid & 3) * 4;
      Bs[k][n] = rb.x; Bs[k + 1][n] = rb.y; Bs[k + 2][n] = rb.z; Bs[k + 3][n] = rb.w;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < KL; k0 += TK) {
    park();
    __syncthreads();
    if (k0 + TK < KL) fetch(k0 + TK);
#pragma unroll
    for (int ks = 0; ks < TK; ks += 4) {
      const int kq = ks + (lane >> 4);
      float fa[4], fb[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = As[kq][wm + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = Bs[kq][wn + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  gemm_tile_store(p, pc, acc, m0 + wm, n0 + wn, lane);
}

// ---- the same product with 16-bit operands: A and B are rounded to T (bf16 | f16) on their way into LDS and multiplied with
// v_mfma_f32_16x16x32_{bf16,f16} (fp32 accumulation, 16 x the rate of the fp32 matrix instruction). Same tile, strides,
// batching, split-K and epilogue as gemm_f32_kernel; K in chunks of 32. SCALAR (= p.scalar: any dimension, stride or
// alignment, e.g. the per-head products of a 171 / 170 split) stages element by element with per-element bounds checks; a
// template parameter, so that the vector form keeps the register budget (and occupancy) of a kernel without that path.
template <typename T, bool SCALAR>
__global__ __launch_bounds__(256) void gemm16_kernel(GemmF32 p) {
  constexpr int TM = 128, TN = 64, TK = 32, LP = TK + 8;              // LP: row pitch in halfwords (80 B: 16-byte aligned rows)
  __shared__ __attribute__((aligned(16))) unsigned short As[TM][LP];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[TN][LP];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 32;
  const GemmBatch z = gemm_tile_batch(p);
  const float *pa = z.pa, *pb = z.pb; float* pc = z.pc; const int KL = z.KL;
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool a_kfast = p.ak == 1, b_nfast = p.bn == 1;
  float4 ra[4], rb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + e * 256;
      int m, k;
      if (a_kfast) { m = idx >> 3; k = (idx & 7) * 4; } else { k = idx >> 5; m = (idx & 31) * 4; }
      const int gm = m0 + m, gk = k0 + k;
      if constexpr (!SCALAR) {
        ra[e] = (gm < p.M && gk < KL) ? *reinterpret_cast<const float4*>(pa + (int64_t)gm * p.am + (int64_t)gk * p.ak)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int mm = a_kfast ? gm : gm + q, kk = a_kfast ? gk + q : gk;
          v[q] = (mm < p.M && kk < KL) ? pa[(int64_t)mm * p.am + (int64_t)kk * p.ak] : 0.f;
        }
        ra[e] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int idx = tid + e * 256;
      int n, k;
      if (b_nfast) { k = idx >> 4; n = (idx & 15) * 4; } else { n = idx >> 3; k = (idx & 7) * 4; }
      const int gn = n0 + n, gk = k0 + k;
      if constexpr (!SCALAR) {
        rb[e] = (gn < p.N && gk < KL) ? *reinterpret_cast<const float4*>(pb + (int64_t)gk * p.bk + (int64_t)gn * p.bn)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int nn = b_nfast ? gn + q : gn, kk = b_nfast ? gk : gk + q;
          v[q] = (nn < p.N && kk < KL) ? pb[(int64_t)kk * p.bk + (int64_t)nn * p.bn] : 0.f;
        }
        rb[e] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + e * 256;
      const unsigned short h0 = to16<T>(ra[e].x), h1 = to16<T>(ra[e].y), h2 = to16<T>(ra[e].z), h3 = to16<T>(ra[e].w);
      if (a_kfast) {
        const int m = idx >> 3, k = (idx & 7) * 4;
        *reinterpret_cast<u16x4*>(&As[m][k]) = u16x4{h0, h1, h2, h3};
      } else {
        const int k = idx >> 5, m = (idx & 31) * 4;
        As[m][k] = h0; As[m + 1][k] = h1; As[m + 2][k] = h2; As[m + 3][k] = h3;
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int idx = tid + e * 256;
      const unsigned short h0 = to16<T>(rb[e].x), h1 = to16<T>(rb[e].y), h2 = to16<T>(rb[e].z), h3 = to16<T>(rb[e].w);
      if (b_nfast) {
        const int k = idx >> 4, n = (idx & 15) * 4;
        Bs[n][k] = h0; Bs[n + 1][k] = h1; Bs[n + 2][k] = h2; Bs[n + 3][k] = h3;
      } else {
        const int n = idx >> 3, k = (idx & 7) * 4;
        *reinterpret_cast<u16x4*>(&Bs[n][k]) = u16x4{h0, h1, h2, h3};
      }
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < KL; k0 += TK) {
    park();
    __syncthreads();
    if (k0 + TK < KL) fetch(k0 + TK);
    const int r = lane & 15, g8 = (lane >> 4) * 8;
    u16x8 fa[4], fb[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const u16x8*>(&As[wm + i * 16 + r][g8]);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const u16x8*>(&Bs[wn + j * 16 + r][g8]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
    __syncthreads();
  }
  gemm_tile_store(p, pc, acc, m0 + wm, n0 + wn, lane);
}

// ---- the vector form of gemm16_kernel with a pipelined K loop ("gemm_amp_pipe"): the same argument block, operands, rounding,
// MFMA, assignment of k to lane group and element, ascending 32-wide chunks from the block's own K start and epilogue, so every
// output element runs the same chain of fp32 operations and gets the same bits. What differs is the loop around the MFMAs:
//  - K in episodes of 64 (two MFMA k-steps per fragment set), two LDS buffers, ONE barrier per episode;
//  - the operands of episode t + 1 wait in registers while episode t - 1 is multiplied; they are rounded and written to the
//    other buffer behind the barrier that ends episode t - 1, and the loads of episode t + 2 are issued at once;
//  - a (32 MI) x (32 NJ) tile on 4 waves of MI x NJ MFMA tiles each. 64 x 64 is the one instantiated: 116 VGPRs, 32 KB of LDS,
//    4 workgroups per CU. 128 x 64, 64 x 128 and 128 x 128 (MI, NJ = 4 work as they are) were measured and lost everywhere;
//  - LDS image [row][64 halfwords]: 128-byte rows without padding, the 16-byte slot c (k = 8c .. 8c + 7) of row r stored at slot
//    c ^ ((r >> 1) & 7). A fragment read (ds_read_b128: lanes r = lane & 15 of slot 4s + (lane >> 4)) then finds each of its four
//    16-lane groups on 16 distinct slots, and a k-contiguous operand is written with one 16-byte store per 8 values;
//  - an operand whose ROWS run fastest in memory (A column-major, B row-major) is fetched as a 4 (rows) x ROWS / 16 (k) block per
//    thread, so each row gets ONE 8- or 16-byte LDS store of consecutive k instead of a 2-byte store per element.
// An episode's second k-step is skipped when it lies past KL, as gemm16_kernel never runs a chunk that starts there.
__device__ __forceinline__ float f4_at(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ int pipe_slot(int row, int c) { return row * 64 + ((c ^ ((row >> 1) & 7)) << 3); }    // in halfwords

// this thread's share of a ROWS x 64 operand tile: element (row, k) at base[row * rs + k * ks], zeros past `rows` and KL
template <int ROWS>
__device__ __forceinline__ void pipe_fetch(float4 (&v)[ROWS / 16], const float* base, int64_t rs, int64_t ks, bool kfast, int row0,
                                           int rows, int k0, int KL, int tid) {
  constexpr int KPT = ROWS / 16, LM = ROWS / 4;
  if (kfast) {
#pragma unroll
    for (int e = 0; e < ROWS / 32; ++e)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int gr = row0 + (tid >> 3) + 32 * e, gk = k0 + (tid & 7) * 8 + 4 * h;
        v[2 * e + h] = (gr < rows && gk < KL) ? *reinterpret_cast<const float4*>(base + (int64_t)gr * rs + gk) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  } else {
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int gr = row0 + (tid % LM) * 4, gk = k0 + (tid / LM) * KPT + i;
      v[i] = (gr < rows && gk < KL) ? *reinterpret_cast<const float4*>(base + (int64_t)gk * ks + gr) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}
template <typename T, int ROWS>
__device__ __forceinline__ void pipe_park(unsigned short* s, const float4 (&v)[ROWS / 16], bool kfast, int tid) {
  constexpr int KPT = ROWS / 16, LM = ROWS / 4;
  if (kfast) {
#pragma unroll
    for (int e = 0; e < ROWS / 32; ++e) {
      const float4 lo = v[2 * e], hi = v[2 * e + 1];
      *reinterpret_cast<u16x8*>(s + pipe_slot((tid >> 3) + 32 * e, tid & 7)) =
          u16x8{to16<T>(lo.x), to16<T>(lo.y), to16<T>(lo.z), to16<T>(lo.w), to16<T>(hi.x), to16<T>(hi.y), to16<T>(hi.z), to16<T>(hi.w)};
    }
  } else {
    const int kb = tid / LM;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (tid % LM) * 4 + j;
      if constexpr (KPT == 8) {
        *reinterpret_cast<u16x8*>(s + pipe_slot(row, kb)) =
            u16x8{to16<T>(f4_at(v[0], j)), to16<T>(f4_at(v[1], j)), to16<T>(f4_at(v[2], j)), to16<T>(f4_at(v[3], j)),
                  to16<T>(f4_at(v[4], j)), to16<T>(f4_at(v[5], j)), to16<T>(f4_at(v[6], j)), to16<T>(f4_at(v[7], j))};
      } else {
        static_assert(KPT == 4, "ROWS is 128 or 64");
        *reinterpret_cast<u16x4*>(s + pipe_slot(row, kb >> 1) + (kb & 1) * 4) =
            u16x4{to16<T>(f4_at(v[0], j)), to16<T>(f4_at(v[1], j)), to16<T>(f4_at(v[2], j)), to16<T>(f4_at(v[3], j))};
      }
    }
  }
}

template <typename T, int MI, int NJ>
__global__ __launch_bounds__(256, MI * NJ <= 4 ? 4 : 1) void gemm16_pipe_kernel(GemmF32 p) {
  constexpr int TM = 32 * MI, TN = 32 * NJ, BK = 64;
  static_assert((TM == 128 || TM == 64) && (TN == 128 || TN == 64), "pipe_fetch / pipe_park cover 128 and 64 rows");
  __shared__ __attribute__((aligned(16))) unsigned short S[2][(TM + TN) * BK];      // [buffer][A rows, then B rows][64]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int wm = (wid >> 1) * (16 * MI), wn = (wid & 1) * (16 * NJ);
  const GemmBatch z = gemm_tile_batch(p);
  const float *pa = z.pa, *pb = z.pb; float* pc = z.pc; const int KL = z.KL;
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool a_kfast = p.ak == 1, b_kfast = p.bn != 1;
  float4 ra[TM / 16], rb[TN / 16];
  auto fetch = [&](int t) {
    pipe_fetch<TM>(ra, pa, p.am, p.ak, a_kfast, m0, p.M, t * BK, KL, tid);
    pipe_fetch<TN>(rb, pb, p.bn, p.bk, b_kfast, n0, p.N, t * BK, KL, tid);
  };
  auto park = [&](int buf) {
    pipe_park<T, TM>(S[buf], ra, a_kfast, tid);
    pipe_park<T, TN>(S[buf] + TM * BK, rb, b_kfast, tid);
  };
  const int nt = (KL + BK - 1) / BK;
  fetch(0);
  park(0);
  if (nt > 1) fetch(1);
  __syncthreads();
  const int r = lane & 15, q = lane >> 4;
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {                     // every wave is past the barrier behind episode t - 1, the last reader of this buffer
      park((t + 1) & 1);
      if (t + 2 < nt) fetch(t + 2);
    }
    const unsigned short *As = S[t & 1], *Bs = As + TM * BK;
    const int steps = t * BK + 32 < KL ? 2 : 1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s < steps) {
        u16x8 fa[MI], fb[NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const u16x8*>(As + pipe_slot(wm + i * 16 + r, 4 * s + q));
#pragma unroll
        for (int j = 0; j < NJ; ++j) fb[j] = *reinterpret_cast<const u16x8*>(Bs + pipe_slot(wn + j * 16 + r, 4 * s + q));
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
      }
    }
    __syncthreads();
  }
  gemm_tile_store(p, pc, acc, m0 + wm, n0 + wn, lane);
}

// The per-thread switches and launch counters of the training path, indexed by TrainInt (train_dev.h); vog_train_set_int and
// vog_train_get_int walk this one table. Values 0 .. hi are accepted, anything else is refused and leaves the stored value as
// it was; hi = 0 marks a launch counter, which can only be reset to 0. Every default is 0.
struct TrainIntDef { const char* name; int hi; const char* values; };
static const TrainIntDef TRAIN_INT_DEFS[TRAIN_INTS] = {
    // 16-bit operands for the tile GEMMs of the training path (any non-zero value counts as 1)
    {"bf16_gemm", 1, "0 off, 1 on"},
    // EVERY product of the training path with bf16 | f16 operands (tile, split-K, weight-stream; the BiLSTM recurrence in the
    // fused kernels of vog_lang_f32). Wins over bf16_gemm.
    {"amp", 2, "0 off, 1 bf16, 2 f16"},
    {"f32_products", 0, nullptr},                  // launches of the fp32 product kernels
    // the fp32 BiLSTM recurrence of vog_lang_f32 in one fused launch per (layer, step) for both directions (train_lang.hip:
    // the K-split kernels with fp32 operands); no effect under amp, which has fused kernels of its own
    {"lstm_fused", 1, "0 stepwise, 1 fused"},
    {"lstm_fused_launches", 0, nullptr},           // launches of those kernels
    // under amp, the BiLSTM recurrence of vog_lang_f32 in the kernels that split K over the waves of a workgroup (train_lang.hip)
    // instead of the wave-per-gate tile kernels; no effect with amp = 0, and no effect on the scratch layout
    {"lstm_amp_split", 1, "0 tile, 1 split"},
    {"lstm_amp_split_launches", 0, nullptr},       // launches of those kernels
    // under amp, the vector tile products of gemm_f32_b in gemm16_pipe_kernel (two LDS buffers, 64-wide K episodes, one barrier
    // each) instead of gemm16_kernel<T, false>: the same bits; no effect with amp = 0, and no effect on any scratch size
    {"gemm_amp_pipe", 1, "0 tile, 1 pipe"},
    {"gemm_amp_pipe_launches", 0, nullptr},        // launches of that kernel
    // vog_attn_fused_f32's forward, dQ and dK / dV launches in their pipelined forms (train_attn.hip: fa_*_pipe_kernel = the
    // launch's one body under StreamPipe, two LDS buffers, one barrier per staged tile) instead of fa_fwd_kernel / fa_bwd_q_kernel /
    // fa_bwd_kv_kernel (the same body under StreamPlain; the plain dQ kernel written out): the same bits, the same scratch; no
    // effect unless the caller runs the fused operator
    {"attn_fused_pipe", 1, "0 fused, 1 pipe"},
    {"attn_fused_pipe_launches", 0, nullptr},      // launches of those kernels
    {"attn_vl_launches", 0, nullptr},              // launches of the kernels vog_attn_*_vl add (train_tx.hip: vl_*_kernel)
    // the training path's device fills and copies (dev_zero / dev_copy / dev_copy2d) as kernels instead of hipMemsetAsync /
    // hipMemcpyAsync / hipMemcpy2DAsync: the same bytes; for recording a captured step as kernel nodes only
    {"kernel_fills", 1, "0 runtime calls, 1 kernels"},
};
static thread_local int g_train[TRAIN_INTS] = {};
int& train_int(TrainInt i) { return g_train[i]; }
// the pointer switches (TrainPtr, train_dev.h; vog_train_set_ptr): every default is NULL
static const char* const TRAIN_PTR_NAMES[TRAIN_PTRS] = {"drop_tick"};
static thread_local const void* g_train_ptr[TRAIN_PTRS] = {};
const void*& train_ptr(TrainPtr i) { return g_train_ptr[i]; }
static int train_int_index(const char* name) {
  for (int i = 0; i < TRAIN_INTS; ++i)
    if (strcmp(name, TRAIN_INT_DEFS[i].name) == 0) return i;
  return -1;
}

// ---- dev_zero / dev_copy / dev_copy2d (train_dev.h): 4-byte words, a grid-stride loop
__global__ __launch_bounds__(256) void dev_zero_kernel(unsigned int* p, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}
__global__ __launch_bounds__(256) void dev_copy2d_kernel(unsigned int* dst, int64_t dpitch, const unsigned int* src, int64_t spitch,
                                                         int64_t width, int64_t height) {      // (pitches and width in words)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < width * height; i += (int64_t)gridDim.x * 256)
    dst[(i / width) * dpitch + i % width] = src[(i / width) * spitch + i % width];
}
static unsigned dev_grid(int64_t words) {
  const int64_t b = (words + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b < 4096 ? b : 4096));
}
static bool recording_step() { return g_train[TRAIN_KERNEL_FILLS] != 0; }
int dev_zero(void* p, size_t bytes, hipStream_t st) {
  if (!recording_step()) { VOG_HIP(hipMemsetAsync(p, 0, bytes, st)); return 0; }
  VOG_CHECK_ARG((bytes & 3) == 0 && (((uintptr_t)p) & 3) == 0);
  if (bytes == 0) return 0;
  ::vog::launch(dev_zero_kernel, dim3(dev_grid((int64_t)(bytes / 4))), dim3(256), 0, st, (unsigned int*)p, (int64_t)(bytes / 4));
  VOG_LAUNCH_CHECK();
  return 0;
}
int dev_copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipStream_t st) {
  if (!recording_step()) { VOG_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, st)); return 0; }
  VOG_CHECK_ARG(((dpitch | spitch | width) & 3) == 0 && ((((uintptr_t)dst) | ((uintptr_t)src)) & 3) == 0 && width <= dpitch && width <= spitch);
  if (width == 0 || height == 0) return 0;
  ::vog::launch(dev_copy2d_kernel, dim3(dev_grid((int64_t)(width / 4 * height))), dim3(256), 0, st, (unsigned int*)dst, (int64_t)(dpitch / 4),
                (const unsigned int*)src, (int64_t)(spitch / 4), (int64_t)(width / 4), (int64_t)height);
  VOG_LAUNCH_CHECK();
  return 0;
}
int dev_copy(void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (!recording_step()) { VOG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)); return 0; }
  return dev_copy2d(dst, bytes, src, bytes, bytes, 1, st);
}

static bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// ---- C[M <= 16, N] = A[M, K] . W[N, K]^T (+ bias, relu, accumulate): the recurrent products of the BiLSTM (M = number of
// sentences). A weight-stream kernel: the 128 x 64 tile GEMM above launches N / 64 workgroups that each walk all of K
// (262 us for dh = dG W_hh at cfg 2); here one WAVE owns CPW output columns, reads their weight rows with 16-byte
// loads (1 KiB per wave and instruction, CPW * K / 256 of them in flight) and the M activation rows from LDS.
// T = float: fp32 operands as they are (the instance holds no rounding code). T = BF16 | F16 (amp mode): both operands are
// rounded to T behind their loads; a product of two 16-bit values is exact in fp32 and the sums stay fp32 - the numerics of the
// 16-bit matrix instruction.
template <typename T> __device__ __forceinline__ float rnd16(float v) { return from16<T>(to16<T>(v)); }
template <int MT, int CPW, typename T>
__global__ __launch_bounds__(256) void skinny_kernel(GemmF32 p) {
  constexpr int KC = 1024;
  constexpr bool R16 = !std::is_same<T, float>::value;
  __shared__ __attribute__((aligned(16))) float As[MT][KC];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = (blockIdx.x * 4 + wid) * CPW;
  float acc[CPW][MT];
#pragma unroll
  for (int c = 0; c < CPW; ++c)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[c][m] = 0.f;
  for (int k0 = 0; k0 < p.K; k0 += KC) {
    const int kc = p.K - k0 < KC ? p.K - k0 : KC;
    __syncthreads();
    for (int i = tid * 4; i < MT * KC; i += 256 * 4) {
      const int m = i / KC, k = i % KC;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < p.M && k < kc) {
        v = *reinterpret_cast<const float4*>(p.a + (int64_t)m * p.am + k0 + k);
        if constexpr (R16) v = make_float4(rnd16<T>(v.x), rnd16<T>(v.y), rnd16<T>(v.z), rnd16<T>(v.w));
      }
      *reinterpret_cast<float4*>(&As[m][k]) = v;
    }
    __syncthreads();
    for (int kk = lane * 4; kk < kc; kk += 256) {
      float4 w[CPW];
#pragma unroll
      for (int c = 0; c < CPW; ++c) {
        w[c] = (n0 + c < p.N) ? *reinterpret_cast<const float4*>(p.b + (int64_t)(n0 + c) * p.bn + k0 + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (R16) w[c] = make_float4(rnd16<T>(w[c].x), rnd16<T>(w[c].y), rnd16<T>(w[c].z), rnd16<T>(w[c].w));
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float4 a = *reinterpret_cast<const float4*>(&As[m][kk]);
#pragma unroll
        for (int c = 0; c < CPW; ++c) acc[c][m] += a.x * w[c].x + a.y * w[c].y + a.z * w[c].z + a.w * w[c].w;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CPW; ++c)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float v = acc[c][m];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0 && m < p.M && n0 + c < p.N) {
        if (p.bias) v += p.bias[n0 + c];
        if (p.relu) v = v < 0.f ? 0.f : v;
        float* dst = p.c + (int64_t)m * p.ldc + n0 + c;
        *dst = p.accum ? *dst + v : v;
      }
    }
}

// out[n, k] = in[k, n]  (W_hh^T for the backward recurrence, once per layer, direction and step() call)
__global__ __launch_bounds__(256) void transpose_f32_kernel(const float* in, float* out, int rows, int cols) {
  __shared__ float t[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8)
    if (by + j < rows && bx + tx < cols) t[j][tx] = in[(int64_t)(by + j) * cols + bx + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (bx + j < cols && by + tx < rows) out[(int64_t)(bx + j) * rows + by + tx] = t[tx][j];
}

void transpose_f32(const float* in, float* out, int rows, int cols, hipStream_t st) {
  ::vog::launch(transpose_f32_kernel, dim3(ceil_div(cols, 32), ceil_div(rows, 32)), dim3(256), 0, st, in, out, rows, cols);
}

// out = (accum ? out : 0) + sum_z part[z] (+ bias, relu), z in order: the second half of a split-K product
__global__ void splitk_reduce_kernel(const float* part, int S, float* c, int64_t ldc, const float* bias, int relu, int accum, int M, int N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int n = (int)(i % N);
  const int64_t m = i / N;
  float v = 0.f;
  for (int z = 0; z < S; ++z) v += part[(int64_t)z * M * N + i];
  if (bias) v += bias[n];
  if (relu) v = v < 0.f ? 0.f : v;
  float* dst = c + m * ldc + n;
  *dst = accum ? *dst + v : v;
}

// partial products of split-K launches: one buffer per stream, grown on demand (training path only). A captured graph keeps the
// buffer's address, so it must not move under one: while the stream is PINNED (vog_train_pin_scratch) or capturing, a request
// beyond the buffer is an error (-3, with a message) that neither allocates nor frees.
struct SplitkBuf { float* ptr = nullptr; size_t bytes = 0; bool pinned = false; };
static std::mutex g_splitk_mu;
static std::map<hipStream_t, SplitkBuf>& splitk_bufs() { static std::map<hipStream_t, SplitkBuf> bufs; return bufs; }
static int splitk_scratch(hipStream_t st, size_t bytes, float** out) {
  std::lock_guard<std::mutex> g(g_splitk_mu);
  SplitkBuf& b = splitk_bufs()[st];
  if (b.bytes < bytes) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (b.pinned || cs != hipStreamCaptureStatusNone)
      VOG_FAIL(-3, "gemm_f32: split-K partials of %zu bytes, the stream's buffer holds %zu and is %s: it cannot grow", bytes, b.bytes,
               b.pinned ? "pinned (vog_train_pin_scratch)" : "being captured");
    if (b.ptr) { (void)hipStreamSynchronize(st); (void)hipFree(b.ptr); }
    b.ptr = nullptr; b.bytes = 0;
    const size_t want = bytes < ((size_t)16 << 20) ? ((size_t)16 << 20) : bytes;
    if (hipMalloc(&b.ptr, want) != hipSuccess) { b.ptr = nullptr; VOG_FAIL(-3, "gemm_f32: no memory for %zu bytes of split-K partials", bytes); }
    b.bytes = want;
  }
  *out = b.ptr;
  return 0;
}

template <typename T>
static void launch_skinny(const GemmF32& p, int M, int N, hipStream_t st) {
  const bool wide = N >= 2048;
  const int cols_per_wg = 4 * (wide ? 4 : 1);
  const dim3 grid(ceil_div(N, cols_per_wg));
  auto go = [&](auto kern, dim3 g) { ::vog::launch(kern, g, dim3(256), 0, st, p); };
  if (M <= 4) { if (wide) go(skinny_kernel<4, 4, T>, grid); else go(skinny_kernel<4, 1, T>, grid); }
  else if (M <= 8) { if (wide) go(skinny_kernel<8, 4, T>, grid); else go(skinny_kernel<8, 1, T>, grid); }
  else { if (wide) go(skinny_kernel<16, 2, T>, dim3(ceil_div(N, 8))); else go(skinny_kernel<16, 1, T>, grid); }
}

// batched form; the vector path is chosen when every dimension, stride and pointer allows 16-byte loads
int gemm_f32_b(const float* a, int64_t am, int64_t ak, int64_t sa, const float* b, int64_t bk, int64_t bn, int64_t sb,
                      float* c, int64_t ldc, int64_t sc, const float* bias, int relu, int accum, int M, int N, int K, int batch,
                      hipStream_t st) {
  VOG_CHECK_ARG((am == 1 || ak == 1) && (bk == 1 || bn == 1) && M > 0 && N > 0 && K > 0 && batch > 0);
  auto m4 = [](int64_t v) { return (v & 3) == 0; };
  const bool vec = m4(M) && m4(N) && m4(K) && (m4(am) || am == 1) && (m4(ak) || ak == 1) && (m4(bk) || bk == 1) &&
                   (m4(bn) || bn == 1) && m4(sa) && m4(sb) && al16(a) && al16(b);
  GemmF32 p{a, am, ak, b, bk, bn, c, ldc, bias, relu, M, N, K, sa, sb, sc, accum, vec ? 0 : 1, 0};
  // the one place that picks the operand type of a product: amp (bf16 | f16, every operand layout), bf16_gemm (vector tiles
  // only), else fp32
  const int amp = g_train[TRAIN_AMP];
  auto tile = [&](const GemmF32& q, dim3 grid) {
    auto tile16 = [&](auto t) {
      using T = decltype(t);
      if (q.scalar) ::vog::launch(gemm16_kernel<T, true>, grid, dim3(256), 0, st, q);
      else ::vog::launch(gemm16_kernel<T, false>, grid, dim3(256), 0, st, q);
    };
    // "gemm_amp_pipe": the pipelined kernel takes every vector call of amp, always on its 64 x 64 tile (the 128-row tiles lost
    // at every shape measured, chip-filling grids included: DESIGN section 4); `grid` only lends its z.
    auto pipe16 = [&](auto t) {
      ::vog::launch(gemm16_pipe_kernel<decltype(t), 2, 2>, dim3(ceil_div(q.N, 64), ceil_div(q.M, 64), grid.z), dim3(256), 0, st, q);
      ++g_train[TRAIN_GEMM_AMP_PIPE_LAUNCHES];
    };
    if (amp && g_train[TRAIN_GEMM_AMP_PIPE] && !q.scalar) amp_type(amp, pipe16);
    else if (amp) amp_type(amp, tile16);
    else if (g_train[TRAIN_BF16_GEMM] && !q.scalar) tile16(BF16{});
    else { ::vog::launch(gemm_f32_kernel, grid, dim3(256), 0, st, q); ++g_train[TRAIN_F32_PRODUCTS]; }
  };
  if (batch == 1 && M <= 16 && ak == 1 && bk == 1 && m4(K) && m4(am) && m4(bn) && al16(a) && al16(b) && N >= 256) {
    // few rows against a K-contiguous weight matrix: weight-stream kernel (one wave per 1 / 4 output columns)
    if (amp) amp_type(amp, [&](auto t) { launch_skinny<decltype(t)>(p, M, N, st); });
    else { launch_skinny<float>(p, M, N, st); ++g_train[TRAIN_F32_PRODUCTS]; }
    VOG_LAUNCH_CHECK();
    return 0;
  }
  const int tiles = ceil_div(N, 64) * ceil_div(M, 128);
  if (batch == 1 && tiles <= 96 && K >= 1024) {
    // few output tiles, long K (the weight gradients: K = rows of the batch): split K over the chip, fixed-order reduction
    int S = 256 / tiles; if (S > K / 256) S = K / 256; if (S > 32) S = 32;
    if (S >= 2) {
      const int kchunk = ceil_div(ceil_div(K, S), 16) * 16;
      S = ceil_div(K, kchunk);
      float* part = nullptr;
      VOG_TRY(splitk_scratch(st, (size_t)S * M * N * 4, &part));
      GemmF32 q = p;
      q.c = part; q.ldc = N; q.bias = nullptr; q.relu = 0; q.accum = 0; q.kchunk = kchunk;
      q.sa = (int64_t)kchunk * ak; q.sb = (int64_t)kchunk * bk; q.sc = (int64_t)M * N;
      if (!(m4(q.sa) && m4(q.sb))) q.scalar = 1;
      tile(q, dim3(ceil_div(N, 64), ceil_div(M, 128), S));
      ::vog::launch(splitk_reduce_kernel, dim3((unsigned)(((int64_t)M * N + 255) / 256)), dim3(256), 0, st, (const float*)part, S, c, ldc,
                    bias, relu, accum, M, N);
      VOG_LAUNCH_CHECK();
      return 0;
    }
  }
  tile(p, dim3(ceil_div(N, 64), ceil_div(M, 128), batch));
  VOG_LAUNCH_CHECK();
  return 0;
}
int gemm_f32(const float* a, int64_t am, int64_t ak, const float* b, int64_t bk, int64_t bn, float* c, int64_t ldc,
                    const float* bias, int relu, int M, int N, int K, hipStream_t st, int accum) {
  return gemm_f32_b(a, am, ak, 0, b, bk, bn, 0, c, ldc, 0, bias, relu, accum, M, N, K, 1, st);
}

}  // namespace vog

using namespace vog;

extern "C" int vog_train_set_int(const char* name, int value) {
  VOG_CHECK_ARG(name);
  const int i = train_int_index(name);
  if (i < 0) VOG_FAIL(-1, "vog_train_set_int: unknown option %s", name);
  const TrainIntDef& d = TRAIN_INT_DEFS[i];
  if (i == TRAIN_BF16_GEMM) value = value ? 1 : 0;
  if (d.hi == 0 && value != 0) VOG_FAIL(-1, "vog_train_set_int: %s can only be reset to 0", name);
  if (value < 0 || value > d.hi) VOG_FAIL(-1, "vog_train_set_int: %s = %d (%s)", name, value, d.values);
  g_train[i] = value;
  return 0;
}

extern "C" int vog_train_get_int(const char* name, int* value) {
  VOG_CHECK_ARG(name && value);
  const int i = train_int_index(name);
  if (i < 0) VOG_FAIL(-1, "vog_train_get_int: unknown option %s", name);
  *value = g_train[i];
  return 0;
}

extern "C" int vog_train_set_ptr(const char* name, const void* value) {
  VOG_CHECK_ARG(name);
  for (int i = 0; i < TRAIN_PTRS; ++i)
    if (strcmp(name, TRAIN_PTR_NAMES[i]) == 0) {
      if ((uintptr_t)value & 7) VOG_FAIL(-1, "vog_train_set_ptr: %s is not 8-byte aligned", name);
      g_train_ptr[i] = value;
      return 0;
    }
  VOG_FAIL(-1, "vog_train_set_ptr: unknown option %s", name);
}

extern "C" int vog_train_pin_scratch(void* stream, int on) {
  std::lock_guard<std::mutex> g(g_splitk_mu);
  splitk_bufs()[(hipStream_t)stream].pinned = on != 0;
  return 0;
}

extern "C" int vog_train_scratch_info(void* stream, void** ptr, size_t* bytes, int* pinned) {
  std::lock_guard<std::mutex> g(g_splitk_mu);
  auto& bufs = splitk_bufs();
  auto it = bufs.find((hipStream_t)stream);
  if (ptr) *ptr = it == bufs.end() ? nullptr : (void*)it->second.ptr;
  if (bytes) *bytes = it == bufs.end() ? 0 : it->second.bytes;
  if (pinned) *pinned = it == bufs.end() ? 0 : (it->second.pinned ? 1 : 0);
  return 0;
}
