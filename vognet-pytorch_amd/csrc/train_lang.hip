// =====================================================================================================================
// Language side in fp32: token re-index -> embedding -> packed multi-layer BiLSTM -> lstm_out_feat_proj -> argument
// vectors (code/mdl_vog.py:67-140, 250-283; utils/mdl_srl_utils.py:114-169), forward recomputation and backward
// (back-propagation through time with packed-sequence semantics: a sentence's state is frozen past its length).
// =====================================================================================================================
#include <algorithm>
#include "train_dev.h"

namespace vog {

__global__ void lang_tokens_kernel(const int64_t* words, const int64_t* mask, int64_t* tok, int Bn, int T, int wlen, int mlen, int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bn * T) return;
  const int bn = i / T, t = i % T;
  const int64_t m = mask[(int64_t)bn * mlen + t];
  tok[i] = m >= 0 ? words[(int64_t)bn * wlen + m] : V;
}
__global__ void embed_gather_kernel(const float* emb, const int64_t* tok, float* x, int rows, int E, Drop dr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * E) return;
  x[i] = emb[tok[i / E] * E + i % E] * drop_scale(dr, (unsigned long long)i);      // F.dropout(x, dropout_in) (mdl_srl_utils.py:128)
}
// g_emb[v, c] = sum over the token positions holding v (fixed order)
__global__ void embed_scatter_kernel(const float* dx, const int64_t* tok, float* g, int rows, int E, int nv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nv * E) return;
  const int64_t v = i / E; const int c = (int)(i % E);
  float s = 0.f;
  for (int r = 0; r < rows; ++r) if (tok[r] == v) s += dx[(int64_t)r * E + c];
  g[i] = s;
}
__global__ void vec_add_kernel(const float* a, const float* b, float* o, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}
__global__ void argvec_gather_kernel(const float* full, const int64_t* cap, float* enc, int Bn, int nsrl, int T, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Bn * nsrl * 2 * D) return;
  const int c = (int)(i % (2 * D));
  const int64_t r = i / (2 * D);
  const int64_t bn = r / nsrl;
  const int64_t t = cap[r * 2 + (c >= D ? 1 : 0)];
  enc[i] = full[(bn * T + t) * D + (c >= D ? c - D : c)];
}
__global__ void argvec_scatter_kernel(const float* denc, const int64_t* cap, float* dfull, int Bn, int nsrl, int T, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Bn * T * D) return;
  const int c = (int)(i % D);
  const int64_t r = i / D;
  const int64_t bn = r / T; const int t = (int)(r % T);
  float s = 0.f;
  for (int a = 0; a < nsrl; ++a) {
    const int64_t q = bn * nsrl + a;
    if (cap[q * 2] == t) s += denc[q * 2 * D + c];
    if (cap[q * 2 + 1] == t) s += denc[q * 2 * D + D + c];
  }
  dfull[i] = s;
}

struct LstmStep {
  const float* gpre;      // [Bn, 4R] h_{s-1} W_hh^T
  const float* xg;        // [Bn*T, 4R] x W_ih^T + b_ih + b_hh
  const int64_t* lens;
  float* gates;           // [T, Bn, 4R] activated (i, f, g, o)
  float* c;               // [T+1, Bn, R] slot s+1 = state after step s, slot 0 = 0
  float* h;               // [T+1, Bn, R]
  float* out;             // [Bn, T, 2R]
  int Bn, T, R, s, reverse;
  // backward
  const float* d_out;     // [Bn, T, 2R]
  const float* dh_cur; float* dh_nxt; float* dc;   // [Bn, R]
  float* dGs;             // [T, Bn, 4R] by step
  float* dGp;             // [Bn, T, 4R] by position (zero where a sentence has ended)
};

// The cell of one (sentence bn, unit r) at step s of one direction, shared by the per-step kernels of the fp32 path and the fused
// ones of amp mode, which differ only in where the recurrent product comes from: pre(g) is this unit's entry of gate g of
// h_{s-1} W_hh^T (a callable, so that it is read behind the frozen-step branch as before: as four values the loads moved
// ahead of it and lstm_cell_fwd_kernel took 8 more VGPRs). A sentence past its length len keeps its state and writes zero gates.
template <typename Pre>
__device__ __forceinline__ void lstm_cell_fwd(int len, int s, int reverse, int Bn, int T, int R, float* gates, float* c, float* h, Pre pre,
                                              const float* xg, float* out, int bn, int r) {
  const bool active = s < len;
  const int pos = reverse ? (len - 1 - s > 0 ? len - 1 - s : 0) : s;
  const int64_t st = ((int64_t)s * Bn + bn), st1 = ((int64_t)(s + 1) * Bn + bn);
  float* gt = gates + st * 4 * R;
  if (!active) {
    c[st1 * R + r] = c[st * R + r];
    h[st1 * R + r] = h[st * R + r];
    gt[r] = gt[R + r] = gt[2 * R + r] = gt[3 * R + r] = 0.f;
    return;
  }
  xg += ((int64_t)bn * T + pos) * 4 * R;
  const float gi = sigm(pre(0) + xg[r]), gf = sigm(pre(1) + xg[R + r]);
  const float gg = tanhf(pre(2) + xg[2 * R + r]), go = sigm(pre(3) + xg[3 * R + r]);
  const float cn = gf * c[st * R + r] + gi * gg;
  const float hn = go * tanhf(cn);
  gt[r] = gi; gt[R + r] = gf; gt[2 * R + r] = gg; gt[3 * R + r] = go;
  c[st1 * R + r] = cn;
  h[st1 * R + r] = hn;
  out[((int64_t)bn * T + pos) * 2 * R + (reverse ? R : 0) + r] = hn;
}

// ... and its backward: dh_in is the gradient of state slot s + 1 from the later steps. Writes dG of step s by step and by
// position and updates dc; only zero dGs where the sentence has ended (the caller passes dh_in through to slot s).
__device__ __forceinline__ void lstm_cell_bwd(float dh_in, int len, const float* gates, const float* c, const float* d_out, float* dc,
                                              float* dGs, float* dGp, int Bn, int T, int R, int s, int reverse, int bn, int r) {
  const int64_t i = (int64_t)bn * R + r;
  const bool active = s < len;
  const int pos = reverse ? (len - 1 - s > 0 ? len - 1 - s : 0) : s;
  const int64_t st = ((int64_t)s * Bn + bn), st1 = ((int64_t)(s + 1) * Bn + bn);
  float* gs = dGs + st * 4 * R;
  if (!active) {
    gs[r] = gs[R + r] = gs[2 * R + r] = gs[3 * R + r] = 0.f;
    return;
  }
  const float* gt = gates + st * 4 * R;
  const float gi = gt[r], gf = gt[R + r], gg = gt[2 * R + r], go = gt[3 * R + r];
  const float tc = tanhf(c[st1 * R + r]);
  const float dh = d_out[((int64_t)bn * T + pos) * 2 * R + (reverse ? R : 0) + r] + dh_in;
  const float dcn = dc[i] + dh * go * (1.f - tc * tc);
  const float d_i = dcn * gg * gi * (1.f - gi), d_f = dcn * c[st * R + r] * gf * (1.f - gf);
  const float d_g = dcn * gi * (1.f - gg * gg), d_o = dh * tc * go * (1.f - go);
  dc[i] = dcn * gf;
  gs[r] = d_i; gs[R + r] = d_f; gs[2 * R + r] = d_g; gs[3 * R + r] = d_o;
  float* gp = dGp + ((int64_t)bn * T + pos) * 4 * R;
  gp[r] = d_i; gp[R + r] = d_f; gp[2 * R + r] = d_g; gp[3 * R + r] = d_o;
}

__global__ void lstm_cell_fwd_kernel(LstmStep a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.Bn * a.R) return;
  const int bn = i / a.R, r = i % a.R, R = a.R;
  const float* gp = a.gpre + (int64_t)bn * 4 * R;
  lstm_cell_fwd((int)a.lens[bn], a.s, a.reverse, a.Bn, a.T, R, a.gates, a.c, a.h, [&](int gate) { return gp[gate * R + r]; }, a.xg, a.out, bn, r);
}

__global__ void lstm_cell_bwd_kernel(LstmStep a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.Bn * a.R) return;
  const int bn = i / a.R, r = i % a.R;
  const int len = (int)a.lens[bn];
  const float dcur = a.dh_cur[i];
  // active: 0 + dGs W_hh (the accumulating GEMM behind this kernel); frozen state: the gradient passes through
  a.dh_nxt[i] = a.s < len ? 0.f : dcur;
  lstm_cell_bwd(dcur, len, a.gates, a.c, a.d_out, a.dc, a.dGs, a.dGp, a.Bn, a.T, a.R, a.s, a.reverse, bn, r);
}

// ---- amp mode: the BiLSTM recurrence with 16-bit operands, one launch per (layer, step) for both directions --------------
// W_hh [4R, R] of every layer and direction -> 16-bit copies w16 (same layout: the forward's B operand, K = R contiguous) and
// wt16 = W_hh^T [R, 4R] (the backward's, K = 4R contiguous); once per vog_lang_f32 call. Either output may be NULL.
struct Whh16 { const float* w[8]; unsigned short* w16[8]; unsigned short* wt16[8]; int G, R; };
template <typename T>
__global__ __launch_bounds__(256) void whh16_kernel(Whh16 a) {
  __shared__ float t[32][33];
  const int z = blockIdx.z, bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float* in = a.w[z];
  unsigned short* w16 = a.w16[z];
  unsigned short* wt16 = a.wt16[z];
  for (int j = ty; j < 32; j += 8)
    if (by + j < a.G && bx + tx < a.R) {
      const int64_t o = (int64_t)(by + j) * a.R + bx + tx;
      t[j][tx] = in[o];
      if (w16) w16[o] = to16<T>(t[j][tx]);
    }
  __syncthreads();
  if (wt16)
    for (int j = ty; j < 32; j += 8)
      if (bx + j < a.R && by + tx < a.G) wt16[(int64_t)(bx + j) * a.G + by + tx] = to16<T>(t[tx][j]);
}

// 8 consecutive entries row[k .. k + 8) as an MFMA fragment (zero past n, or everywhere when !ok); vec: 16-byte loads allowed
template <typename T>
__device__ __forceinline__ u16x8 frag8_f32(const float* row, int k, int n, bool ok, bool vec) {
  u16x8 r;
  if (ok && vec && k + 8 <= n) {
    const float4 x = *reinterpret_cast<const float4*>(row + k), y = *reinterpret_cast<const float4*>(row + k + 4);
    r = u16x8{to16<T>(x.x), to16<T>(x.y), to16<T>(x.z), to16<T>(x.w), to16<T>(y.x), to16<T>(y.y), to16<T>(y.z), to16<T>(y.w)};
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (ok && k + j < n) ? to16<T>(row[k + j]) : (unsigned short)0;
  }
  return r;
}
__device__ __forceinline__ u16x8 frag8_u16(const unsigned short* row, int k, int n, bool ok, bool vec) {
  if (ok && vec && k + 8 <= n) return *reinterpret_cast<const u16x8*>(row + k);
  u16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (ok && k + j < n) ? row[k + j] : (unsigned short)0;
  return r;
}

// ---- the fused recurrence: one launch per (layer, step) runs both directions (blockIdx.z): the recurrent product on the
// matrix cores, then the cell of one (sentence, unit) per thread in fp32. Buffers and the frozen state past a sentence's length
// are those of lstm_cell_{fwd,bwd}_kernel. No atomics, no cross-workgroup traffic: a launch reads state slot s (dG of step
// s + 1) and writes slot s + 1 (dG of step s); dh / dc are updated in place by the one thread that owns the element.
// Three forms share these arguments: amp's tile kernels (16-bit operands, the default under amp), and the K-split kernels
// with 16-bit operands ("lstm_amp_split") or fp32 ones ("lstm_fused").
struct LstmRecur {
  const void* w[2];                // per direction; forward: W_hh [4R, R], backward: W_hh^T [R, 4R]; 16-bit (w16 / wt16) or fp32 by the kernel
  const float* xg[2]; float* gates[2]; float* c[2]; float* h[2]; float* out;
  const int64_t* lens; int Bn, T, R, s;
  const float* d_out; float* dh[2]; float* dc[2]; float* dGs[2]; float* dGp[2];
  int first;                       // backward: s = T - 1 (dh holds the gradient that enters at state slot T)
  int wvec;                        // the K-split kernels: 16-byte loads of w allowed (its pointers and row pitch are multiples of 16 bytes)
};

// amp's tile form: a workgroup owns 16 hidden units x 16 sentences; wave g computes gate g's 16 x 16 block of the recurrent
// product over all of K with v_mfma_f32_16x16x32 (fp32 accumulation).
template <typename T>
__global__ __launch_bounds__(256) void lstm_amp_fwd_kernel(LstmRecur a) {
  __shared__ float gl[4][16][17];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int r0 = blockIdx.x * 16, b0 = blockIdx.y * 16, dr = blockIdx.z, R = a.R, Bn = a.Bn;
  const int am = b0 + (lane & 15), wn = r0 + (lane & 15), kq = (lane >> 4) * 8;
  const float* arow = a.h[dr] + ((int64_t)a.s * Bn + am) * R;                   // h_{s-1}: state slot s
  const unsigned short* brow = (const unsigned short*)a.w[dr] + ((int64_t)g * R + wn) * R;   // W_hh row of gate g, unit wn
  const bool aok = am < Bn, bok = wn < R, avec = (R & 3) == 0, bvec = (R & 7) == 0;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < R; k0 += 32)
    acc = mfma16<T>(frag8_f32<T>(arow, k0 + kq, R, aok, avec), frag8_u16(brow, k0 + kq, R, bok, bvec), acc);
#pragma unroll
  for (int q = 0; q < 4; ++q) gl[g][(lane >> 4) * 4 + q][lane & 15] = acc[q];     // D: row = sentence, col = unit
  __syncthreads();
  const int m = tid >> 4, u = tid & 15, bn = b0 + m, r = r0 + u;
  if (bn >= Bn || r >= R) return;
  lstm_cell_fwd((int)a.lens[bn], a.s, dr, Bn, a.T, R, a.gates[dr], a.c[dr], a.h[dr], [&](int gate) { return gl[gate][m][u]; }, a.xg[dr], a.out,
                bn, r);
}

// dh (the gradient of state slot s + 1) = dG_{s+1} W_hh from wt16 (K = 4R split over the 4 waves, summed in fixed order), or
// the gradient passed through a frozen step; then the cell backward of step s. dh / dc are updated in place per element.
template <typename T>
__global__ __launch_bounds__(256) void lstm_amp_bwd_kernel(LstmRecur a) {
  __shared__ float red[4][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * 16, b0 = blockIdx.y * 16, dr = blockIdx.z, R = a.R, Bn = a.Bn, G = 4 * R;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!a.first) {
    const int am = b0 + (lane & 15), wn = r0 + (lane & 15), kq = (lane >> 4) * 8;
    const float* arow = a.dGs[dr] + ((int64_t)(a.s + 1) * Bn + am) * G;
    const unsigned short* brow = (const unsigned short*)a.w[dr] + (int64_t)wn * G;
    const bool aok = am < Bn, bok = wn < R, bvec = (G & 7) == 0;
    const int kc = (G / 4 + 31) / 32 * 32, k1 = (wv + 1) * kc < G ? (wv + 1) * kc : G;
    for (int k0 = wv * kc; k0 < k1; k0 += 32)
      acc = mfma16<T>(frag8_f32<T>(arow, k0 + kq, G, aok, true), frag8_u16(brow, k0 + kq, G, bok, bvec), acc);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wv][(lane >> 4) * 4 + q][lane & 15] = acc[q];
  __syncthreads();
  const int m = tid >> 4, u = tid & 15, bn = b0 + m, r = r0 + u;
  if (bn >= Bn || r >= R) return;
  const int64_t i = (int64_t)bn * R + r;
  const int len = (int)a.lens[bn];
  float* dhp = a.dh[dr];
  // step s + 1 active: dh = dG_{s+1} W_hh; frozen (its dG row is zero): the gradient passes through
  const float dcur = a.first ? dhp[i] : ((red[0][m][u] + red[1][m][u]) + (red[2][m][u] + red[3][m][u])) + (a.s + 1 < len ? 0.f : dhp[i]);
  dhp[i] = dcur;
  lstm_cell_bwd(dcur, len, a.gates[dr], a.c[dr], a.d_out, a.dc[dr], a.dGs[dr], a.dGp[dr], Bn, a.T, R, a.s, dr, bn, r);
}

// ---- the K-split form: the same two steps with K split over the waves of a workgroup ("lstm_amp_split", "lstm_fused") --------
// Where the tile kernels give a wave a whole 16 x 16 block and all of K, here a wave sums its chunk of K, the partial 16 x 16
// accumulators meet in LDS and are added in wave order, so that a workgroup owns fewer units and the grid fills the chip at
// R = 1024. One forward and one backward body (lstm_ksplit_{fwd,bwd}_kernel below); what a wave multiplies is an operand
// policy: Op16<T> - h / dG rounded per fragment from fp32, W_hh from w16 / wt16, v_mfma_f32_16x16x32, the operands and rounding
// of the tile kernels under another order of the fp32 sums - or OpF32 - exact fp32 products on v_mfma_f32_16x16x4_f32.

// U whole steps of 32 at a time while they fit under k1, from k on: the 3 U loads of a batch (16 bytes each, no conditions) are
// issued ahead of its U MFMAs, which run in k order. arow / brow already point at the lane's 8 entries of step 0.
// (A `#pragma unroll` over the guarded fragments instead compiled to one load, one wait and one MFMA per trip.)
template <typename T, int U>
__device__ __forceinline__ f32x4 split_steps(const float* arow, const unsigned short* brow, int& k, int k1, f32x4 acc) {
  for (; k + 32 * U <= k1; k += 32 * U) {              // U whole steps at a time: 3 U loads, then U MFMAs in k order
    float4 x[U], y[U];
    u16x8 fb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      x[u] = *reinterpret_cast<const float4*>(arow + k + 32 * u);
      y[u] = *reinterpret_cast<const float4*>(arow + k + 32 * u + 4);
      fb[u] = *reinterpret_cast<const u16x8*>(brow + k + 32 * u);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const u16x8 fa = u16x8{to16<T>(x[u].x), to16<T>(x[u].y), to16<T>(x[u].z), to16<T>(x[u].w),
                             to16<T>(y[u].x), to16<T>(y[u].y), to16<T>(y[u].z), to16<T>(y[u].w)};
      acc = mfma16<T>(fa, fb[u], acc);
    }
  }
  return acc;
}
// acc += A[16, k0 .. k1) B[k0 .. k1, 16] of one wave; k0 a multiple of 32, k1 <= n (nothing when k0 >= k1). arow / brow point at
// rows that exist (the caller clamps them); aok / bok say whether they are this lane's own. Where 16-byte loads are allowed
// (avec, bvec) the whole steps are loaded without conditions - a row that is not the lane's own then fills an output row or
// column that nobody reads - in batches of U, then one by one; the rest (a partial step, element loads, zeros past n) goes
// through the guarded fragments.
template <typename T, int U>
__device__ __forceinline__ f32x4 split_product(const float* arow, const unsigned short* brow, int k0, int k1, int n, int kq, bool aok,
                                               bool bok, bool avec, bool bvec, f32x4 acc) {
  int k = k0;
  if (avec && bvec) {
    acc = split_steps<T, U>(arow + kq, brow + kq, k, k1, acc);
    acc = split_steps<T, 1>(arow + kq, brow + kq, k, k1, acc);
  }
  for (; k < k1; k += 32) acc = mfma16<T>(frag8_f32<T>(arow, k + kq, n, aok, avec), frag8_u16(brow, k + kq, n, bok, bvec), acc);
  return acc;
}

// row[k .. k + 4) (zero past n, or everywhere when !ok); vec: a 16-byte load is allowed
__device__ __forceinline__ float4 ld4_f32(const float* row, int k, int n, bool ok, bool vec) {
  if (ok && vec && k + 4 <= n) return *reinterpret_cast<const float4*>(row + k);
  float4 r;
  r.x = (ok && k < n) ? row[k] : 0.f; r.y = (ok && k + 1 < n) ? row[k + 1] : 0.f;
  r.z = (ok && k + 2 < n) ? row[k + 2] : 0.f; r.w = (ok && k + 3 < n) ? row[k + 3] : 0.f;
  return r;
}
// acc += A[16, k0 .. k0 + 16) B[k0 .. k0 + 16, 16] from one 16-byte load per lane and operand: lane (q = lane / 16, i = lane % 16)
// holds entries k0 + 4q .. 4q + 3 of row i of A and of column i of B, so MFMA j multiplies the k = k0 + 4q + j of every q
__device__ __forceinline__ f32x4 mfma_k16(float4 x, float4 y, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, y.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, y.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, y.z, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, y.w, acc, 0, 0, 0);
}

// The operand policies: the element type W of the weight rows, the K of one step (a wave's chunk of K is rounded up to a
// multiple of it) of which a lane holds KLANE entries per operand from lane / 16 * KLANE on, and
// product: acc += A[16, k0 .. k1) B[k0 .. k1, 16] of one wave; k0 a multiple of KSTEP, k1 <= n (nothing when k0 >= k1).
// arow / brow point at row(i, ok, n) of their operand; aok / bok say whether row i < n is there, and so the lane's own.
// No load leaves the rows that exist: OpF32 guards every load with ok and forms the pointer as it is; Op16's batched loads
// have no conditions, so it clamps a missing row to the last real one.
struct OpF32 {
  using W = float;
  static constexpr int KSTEP = 16, KLANE = 4;
  static __device__ __forceinline__ int row(int i, bool ok, int n) { return i; }
  static __device__ __forceinline__ f32x4 product(const float* arow, const float* brow, int k0, int k1, int n, int kq, bool aok, bool bok,
                                                  bool avec, bool bvec, f32x4 acc) {
#pragma unroll 4
    for (int k = k0; k < k1; k += KSTEP) acc = mfma_k16(ld4_f32(arow, k + kq, n, aok, avec), ld4_f32(brow, k + kq, n, bok, bvec), acc);
    return acc;
  }
};
template <typename T>
struct Op16 {
  using W = unsigned short;
  static constexpr int KSTEP = 32, KLANE = 8;
  static __device__ __forceinline__ int row(int i, bool ok, int n) { return ok ? i : n - 1; }
  static __device__ __forceinline__ f32x4 product(const float* arow, const unsigned short* brow, int k0, int k1, int n, int kq, bool aok,
                                                  bool bok, bool avec, bool bvec, f32x4 acc) {
    return split_product<T, 8>(arow, brow, k0, k1, n, kq, aok, bok, avec, bvec, acc);
  }
};

// Forward: a workgroup owns UNITS hidden units x 4 gates (the 16 columns of one MFMA tile: column = gate * UNITS + unit) x 16
// sentences; its WAVES waves split K = R. 16 UNITS threads then apply the cell of one (sentence, unit) each. At 4 units and
// 4 waves: 512 workgroups at R = 1024 where the tile kernel has 128, and with 16-bit operands a chain of 8 MFMAs per wave
// instead of 32.
// Backward: dh (the gradient of state slot s + 1) = dG_{s+1} W_hh from W_hh^T (K = 4R contiguous), or the gradient passed through
// a frozen step, then the cell backward of step s, as lstm_amp_bwd_kernel does it. A workgroup owns UNITS = 16 hidden units x 16
// sentences as there, but 16 waves split K = 4R instead of 4. N = R gives only R / 16 workgroups per direction (128 in all at
// R = 1024), so the waves, not the workgroups, put enough loads in flight: in fp32, 16 waves measured 6.5 us per launch under
// 8, and 8 units per workgroup (256 workgroups, half of every B fragment unused) measured the same as 16 at either wave count.
constexpr int KF_UNITS = 4, KF_WAVES = 4, KB_UNITS = 16, KB_WAVES = 16;

template <typename Op, int UNITS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void lstm_ksplit_fwd_kernel(LstmRecur a) {
  static_assert(4 * UNITS == 16, "the 4 gates of a workgroup's units are the 16 columns of one MFMA tile");
  __shared__ float red[WAVES][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * UNITS, b0 = blockIdx.y * 16, dr = blockIdx.z, R = a.R, Bn = a.Bn;
  const int col = lane & 15, am = b0 + col, wn = r0 + col % UNITS, kq = (lane >> 4) * Op::KLANE;
  const bool aok = am < Bn, bok = wn < R;
  const float* arow = a.h[dr] + ((int64_t)a.s * Bn + Op::row(am, aok, Bn)) * R;                      // h_{s-1}: state slot s
  const typename Op::W* brow = (const typename Op::W*)a.w[dr] + ((int64_t)(col / UNITS) * R + Op::row(wn, bok, R)) * R;   // W_hh row of gate col / UNITS, unit wn
  const int kc = ((R + WAVES - 1) / WAVES + Op::KSTEP - 1) / Op::KSTEP * Op::KSTEP, k1 = (wv + 1) * kc < R ? (wv + 1) * kc : R;
  const f32x4 acc = Op::product(arow, brow, wv * kc, k1, R, kq, aok, bok, (R & 3) == 0, a.wvec != 0, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wv][(lane >> 4) * 4 + q][col] = acc[q];          // D: row = sentence, col = gate * UNITS + unit
  __syncthreads();
  if (tid >= 16 * UNITS) return;
  const int m = tid / UNITS, u = tid % UNITS, bn = b0 + m, r = r0 + u;
  if (bn >= Bn || r >= R) return;
  lstm_cell_fwd((int)a.lens[bn], a.s, dr, Bn, a.T, R, a.gates[dr], a.c[dr], a.h[dr],
                [&](int gate) {
                  const int n = gate * UNITS + u;
                  float sum = red[0][m][n];
#pragma unroll
                  for (int w = 1; w < WAVES; ++w) sum += red[w][m][n];
                  return sum;
                },
                a.xg[dr], a.out, bn, r);
}

template <typename Op, int UNITS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void lstm_ksplit_bwd_kernel(LstmRecur a) {
  static_assert(UNITS == 16 && 16 * UNITS <= 64 * WAVES, "a unit per column of the MFMA tile, a thread per (sentence, unit)");
  __shared__ float red[WAVES][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * UNITS, b0 = blockIdx.y * 16, dr = blockIdx.z, R = a.R, Bn = a.Bn, G = 4 * R;
  const int col = lane & 15;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!a.first) {
    const int am = b0 + col, wn = r0 + col, kq = (lane >> 4) * Op::KLANE;
    const bool aok = am < Bn, bok = wn < R;
    const float* arow = a.dGs[dr] + ((int64_t)(a.s + 1) * Bn + Op::row(am, aok, Bn)) * G;
    const typename Op::W* brow = (const typename Op::W*)a.w[dr] + (int64_t)Op::row(wn, bok, R) * G;
    const int kc = ((G + WAVES - 1) / WAVES + Op::KSTEP - 1) / Op::KSTEP * Op::KSTEP, k1 = (wv + 1) * kc < G ? (wv + 1) * kc : G;
    acc = Op::product(arow, brow, wv * kc, k1, G, kq, aok, bok, true, a.wvec != 0, acc);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wv][(lane >> 4) * 4 + q][col] = acc[q];
  __syncthreads();
  if (tid >= 16 * UNITS) return;
  const int m = tid / UNITS, u = tid % UNITS, bn = b0 + m, r = r0 + u;
  if (bn >= Bn || r >= R) return;
  const int64_t i = (int64_t)bn * R + r;
  const int len = (int)a.lens[bn];
  float* dhp = a.dh[dr];
  float dcur = dhp[i];
  if (!a.first) {
    float sum = red[0][m][u];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) sum += red[w][m][u];
    // step s + 1 active: dh = dG_{s+1} W_hh; frozen (its dG row is zero): the gradient passes through
    dcur = sum + (a.s + 1 < len ? 0.f : dcur);
  }
  dhp[i] = dcur;
  lstm_cell_bwd(dcur, len, a.gates[dr], a.c[dr], a.d_out, a.dc[dr], a.dGs[dr], a.dGp[dr], Bn, a.T, R, a.s, dr, bn, r);
}

}  // namespace vog

using namespace vog;

struct LangBufs {
  int64_t* tok; float* x0;                             // tokens [Bn*T], embeddings [Bn*T, E]
  float *lout[4], *xg[4][2], *gates[4][2], *cst[4][2], *hst[4][2];   // per layer (and direction): output, x W_ih^T, gates, c, h
  float *gpre, *dGs, *dGp, *dh0, *dh1, *dc, *bsum;
  float *dxa, *dxb;                                    // d_x of a layer: the current layer's d_out / the next one's
  float *full, *dfull, *enc, *denc, *lenc, *dpre; ColPart part;
  float *dpre2, *whh_t;
  float *hfin, *dfin, *hpre, *dpreh;                   // d_hid: final_hidden, its gradient, hid pre-activation, its gradient
  // amp only: 16-bit W_hh / W_hh^T of every layer and direction; the second direction's dGs, dGp, dc (both run at once)
  // (fused fp32 recurrence: the same dGs1, dGp1, dc1, and the second direction's W_hh^T of the layer in hand)
  unsigned short *w16[4][2], *wt16[4][2]; float *dGs1, *dGp1, *dc1, *whh_t1;
  int64_t bytes;
};
static LangBufs lang_layout(void* base, int Bn, int T, int nsrl, int E, int R, int NL, int D, int L, int amp, int fused) {
  Carve c(base, 64, true);
  LangBufs b{};
  const int64_t BT = (int64_t)Bn * T, G = 4 * R, BR = (int64_t)Bn * R, MA = (int64_t)Bn * nsrl;
  b.tok = c.take<int64_t>(BT + 8);
  b.x0 = c.take<float>(BT * E);
  for (int l = 0; l < NL; ++l) {
    b.lout[l] = c.take<float>(BT * 2 * R);
    for (int dr = 0; dr < 2; ++dr) {
      b.xg[l][dr] = c.take<float>(BT * G); b.gates[l][dr] = c.take<float>(BT * G);
      b.cst[l][dr] = c.take<float>((T + 1) * BR); b.hst[l][dr] = c.take<float>((T + 1) * BR);
    }
  }
  b.gpre = c.take<float>(Bn * G);
  b.dGs = c.take<float>(BT * G); b.dGp = c.take<float>(BT * G);
  for (float** p : {&b.dh0, &b.dh1, &b.dc}) *p = c.take<float>(BR);
  b.bsum = c.take<float>(G);
  b.dxa = c.take<float>(BT * std::max(E, 2 * R)); b.dxb = c.take<float>(BT * std::max(E, 2 * R));
  b.full = c.take<float>(BT * D); b.dfull = c.take<float>(BT * D);
  b.enc = c.take<float>(MA * 2 * D); b.denc = c.take<float>(MA * 2 * D);
  b.lenc = c.take<float>(MA * L); b.dpre = c.take<float>(MA * L);
  // the matrices summed by columns: dG [., 4R] (LSTM biases), dpre [., L] (b_arg), dpre2 / dpreh [., D] (b_proj)
  b.part = c.colpart(std::max({4 * R, L, D}));
  b.dpre2 = c.take<float>(BT * D); b.whh_t = c.take<float>(G * R);
  b.hfin = c.take<float>(2 * BR); b.dfin = c.take<float>(2 * BR);
  b.hpre = c.take<float>((int64_t)Bn * D); b.dpreh = c.take<float>((int64_t)Bn * D);
  if (amp)
    for (int l = 0; l < NL; ++l)
      for (int dr = 0; dr < 2; ++dr) {                 // (G * R values and one spare float, as these carves always were)
        b.w16[l][dr] = c.take<unsigned short>(G * R + 2); b.wt16[l][dr] = c.take<unsigned short>(G * R + 2);
      }
  if (amp || fused) { b.dGs1 = c.take<float>(BT * G); b.dGp1 = c.take<float>(BT * G); b.dc1 = c.take<float>(BR); }
  if (!amp && fused) b.whh_t1 = c.take<float>(G * R);
  b.bytes = c.bytes();
  return b;
}
// (the size follows the calling thread's "amp" and "lstm_fused" switches, as the entry's layout does)
extern "C" int64_t vog_lang_f32_scratch_bytes(int Bn, int T, int nsrl, int E, int R, int layers, int D, int L) {
  if (Bn <= 0 || T <= 0 || nsrl <= 0 || E <= 0 || R <= 0 || layers <= 0 || layers > 4 || D <= 0 || L <= 0) return -1;
  return lang_layout(nullptr, Bn, T, nsrl, E, R, layers, D, L, train_amp(), train_int(TRAIN_LSTM_FUSED)).bytes;
}

static dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
static bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// The fused recurrence of layer l (amp, or fp32 under "lstm_fused"): everything but w, wvec, d_out and the step, for the
// forward and the backward alike. Both directions run at once, so the second one has dGs, dGp, dc of its own.
static LstmRecur lstm_recur_args(const vog_lang_f32_args* a, const LangBufs& b, int l) {
  LstmRecur r{};
  float* const dh[2] = {b.dh0, b.dh1};
  float* const dc[2] = {b.dc, b.dc1};
  float* const dGs[2] = {b.dGs, b.dGs1};
  float* const dGp[2] = {b.dGp, b.dGp1};
  for (int d = 0; d < 2; ++d) {
    r.xg[d] = b.xg[l][d]; r.gates[d] = b.gates[l][d]; r.c[d] = b.cst[l][d]; r.h[d] = b.hst[l][d];
    r.dh[d] = dh[d]; r.dc[d] = dc[d]; r.dGs[d] = dGs[d]; r.dGp[d] = dGp[d];
  }
  r.out = b.lout[l]; r.lens = a->lens; r.Bn = a->Bn; r.T = a->T; r.R = a->R;
  return r;
}
// One step of it, forward or backward: amp's tile kernels, the K-split ones with amp's operands (split), or with fp32
// operands (amp = 0). The one place that counts "lstm_fused_launches" and "lstm_amp_split_launches".
template <typename Op>
static void lstm_ksplit_launch(const LstmRecur& r, bool bwd, hipStream_t st) {
  const dim3 grid(ceil_div(r.R, bwd ? KB_UNITS : KF_UNITS), ceil_div(r.Bn, 16), 2);
  if (bwd) ::vog::launch(lstm_ksplit_bwd_kernel<Op, KB_UNITS, KB_WAVES>, grid, dim3(64 * KB_WAVES), 0, st, r);
  else ::vog::launch(lstm_ksplit_fwd_kernel<Op, KF_UNITS, KF_WAVES>, grid, dim3(64 * KF_WAVES), 0, st, r);
}
static void lstm_recur_launch(const LstmRecur& r, int amp, int split, bool bwd, hipStream_t st) {
  if (!amp) {
    lstm_ksplit_launch<OpF32>(r, bwd, st);
    ++train_int(TRAIN_LSTM_FUSED_LAUNCHES);
  } else if (split) {
    amp_type(amp, [&](auto ty) { lstm_ksplit_launch<Op16<decltype(ty)>>(r, bwd, st); });
    ++train_int(TRAIN_LSTM_AMP_SPLIT_LAUNCHES);
  } else {
    const dim3 grid(ceil_div(r.R, 16), ceil_div(r.Bn, 16), 2);
    amp_type(amp, [&](auto ty) {
      if (bwd) ::vog::launch(lstm_amp_bwd_kernel<decltype(ty)>, grid, dim3(256), 0, st, r);
      else ::vog::launch(lstm_amp_fwd_kernel<decltype(ty)>, grid, dim3(256), 0, st, r);
    });
  }
}

// The recurrence of layer l, forward, called once direction dr's input projection and zero state are in place. fp32: the T steps
// of direction dr, each a recurrent product and the cell. amp: one fused launch per step runs both directions, so it waits for
// dr = 1; so does the fused fp32 recurrence ("lstm_fused"). split: amp's launch is the K-split kernel ("lstm_amp_split").
static int lang_recur_fwd(const vog_lang_f32_args* a, const LangBufs& b, int l, int dr, int amp, int fused, int split, hipStream_t st) {
  const int Bn = a->Bn, T = a->T, R = a->R, G = 4 * R;
  if (!amp && !fused) {
    for (int t = 0; t < T; ++t) {
      VOG_TRY(gemm_f32(b.hst[l][dr] + (int64_t)t * Bn * R, R, 1, a->w_hh[l][dr], 1, R, b.gpre, G, nullptr, 0, Bn, G, R, st));
      LstmStep ls{}; ls.gpre = b.gpre; ls.xg = b.xg[l][dr]; ls.lens = a->lens; ls.gates = b.gates[l][dr]; ls.c = b.cst[l][dr];
      ls.h = b.hst[l][dr]; ls.out = b.lout[l]; ls.Bn = Bn; ls.T = T; ls.R = R; ls.s = t; ls.reverse = dr;
      ::vog::launch(lstm_cell_fwd_kernel, blocks((int64_t)Bn * R), dim3(256), 0, st, ls);
    }
    return 0;
  }
  if (dr == 0) return 0;
  LstmRecur r = lstm_recur_args(a, b, l);
  for (int d = 0; d < 2; ++d) r.w[d] = amp ? (const void*)b.w16[l][d] : a->w_hh[l][d];
  r.wvec = (R & (amp ? 7 : 3)) == 0 && al16(r.w[0]) && al16(r.w[1]);                 // rows of R values: 8 of 16 bits | 4 floats
  for (int t = 0; t < T; ++t) {
    r.s = t;
    lstm_recur_launch(r, amp, split, false, st);
  }
  return 0;
}

// ---- forward (re)computation
static int lang_forward(const vog_lang_f32_args* a, const LangBufs& b, int amp, int fused, int split, hipStream_t st) {
  const int Bn = a->Bn, T = a->T, nsrl = a->nsrl, E = a->E, R = a->R, NL = a->layers, D = a->D, L = a->L;
  const int BT = Bn * T, G = 4 * R;
  ::vog::launch(lang_tokens_kernel, blocks(BT), dim3(256), 0, st, a->words_ind, a->word_mask, b.tok, Bn, T, a->words_len, a->mask_len,
                a->vocab_size);
  ::vog::launch(embed_gather_kernel, blocks((int64_t)BT * E), dim3(256), 0, st, a->emb, (const int64_t*)b.tok, b.x0, BT, E,
                make_drop(a->drop_in, a->drop_seed, 1));
  for (int l = 0; l < NL; ++l) {
    const float* xin = l == 0 ? b.x0 : b.lout[l - 1];
    const int K = l == 0 ? E : 2 * R;
    VOG_TRY(dev_zero(b.lout[l], (size_t)BT * 2 * R * 4, st));           // zero past each sentence's length
    for (int dr = 0; dr < 2; ++dr) {
      ::vog::launch(vec_add_kernel, blocks(G), dim3(256), 0, st, a->b_ih[l][dr], a->b_hh[l][dr], b.bsum, G);
      VOG_TRY(gemm_f32(xin, K, 1, a->w_ih[l][dr], 1, K, b.xg[l][dr], G, b.bsum, 0, BT, G, K, st));
      VOG_TRY(dev_zero(b.cst[l][dr], (size_t)Bn * R * 4, st));
      VOG_TRY(dev_zero(b.hst[l][dr], (size_t)Bn * R * 4, st));
      VOG_TRY(lang_recur_fwd(a, b, l, dr, amp, fused, split, st));
    }
    // nn.LSTM's dropout between the layers / F.dropout on the encoder output (mdl_srl_utils.py:104, 150): in place - the
    // recurrence reads its own state buffers, only the next layer / the projection read this tensor
    const Drop dl = make_drop(a->drop_out, a->drop_seed, l < NL - 1 ? 2 + l : 10);
    if (dl.thr) mask_mul(b.lout[l], b.lout[l], dl, (int64_t)BT * 2 * R, st);
  }
  VOG_TRY(gemm_f32(b.lout[NL - 1], 2 * R, 1, a->w_proj, 1, 2 * R, b.full, D, a->b_proj, 1, BT, D, 2 * R, st));   // relu(x W^T + b), every step
  ::vog::launch(argvec_gather_kernel, blocks((int64_t)Bn * nsrl * 2 * D), dim3(256), 0, st, (const float*)b.full, a->capture, b.enc, Bn,
                nsrl, T, D);
  VOG_TRY(gemm_f32(b.enc, 2 * D, 1, a->w_arg, 1, 2 * D, b.lenc, L, a->b_arg, 1, Bn * nsrl, L, 2 * D, st));
  if (a->hid_out) {
    // final_hidden = [h_fwd after the last valid step | h_bwd after its last step (position 0)] of the top layer: the state
    // slot T (frozen past each sentence's length), then the same projection (code/mdl_vog.py:270-283)
    concat_rows(b.hst[NL - 1][0] + (int64_t)T * Bn * R, R, 1, b.hst[NL - 1][1] + (int64_t)T * Bn * R, R, 1, b.hfin, Bn, st);
    VOG_TRY(gemm_f32(b.hfin, 2 * R, 1, a->w_proj, 1, 2 * R, a->hid_out, D, a->b_proj, 1, Bn, D, 2 * R, st));
  }
  if (a->lang_enc_out) VOG_TRY(dev_copy(a->lang_enc_out, b.lenc, (size_t)Bn * nsrl * L * 4, st));
  if (a->full_out) VOG_TRY(dev_copy(a->full_out, b.full, (size_t)BT * D * 4, st));
  return 0;
}

// One direction's start of the backward recurrence of layer l, in both modes: zero dG by position, dh = the gradient that enters
// at state slot T (under d_hid the top layer's half of d final_hidden, else zero), zero dc.
static int lang_bwd_dir_init(const vog_lang_f32_args* a, const LangBufs& b, int l, int dr, float* dGp, float* dh, float* dc, hipStream_t st) {
  const int Bn = a->Bn, R = a->R;
  VOG_TRY(dev_zero(dGp, (size_t)Bn * a->T * 4 * R * 4, st));
  if (a->d_hid && l == a->layers - 1)
    VOG_TRY(dev_copy2d(dh, (size_t)R * 4, b.dfin + dr * R, (size_t)2 * R * 4, (size_t)R * 4, Bn, st));
  else
    VOG_TRY(dev_zero(dh, (size_t)Bn * R * 4, st));
  VOG_TRY(dev_zero(dc, (size_t)Bn * R * 4, st));
  return 0;
}

// ---- backward (back-propagation through time), from d_lang_enc (and d_hid) over the forward that `b` holds
static int lang_backward(const vog_lang_f32_args* a, const LangBufs& b, int amp, int fused, int split, hipStream_t st) {
  const int Bn = a->Bn, T = a->T, nsrl = a->nsrl, E = a->E, R = a->R, NL = a->layers, D = a->D, L = a->L;
  const int BT = Bn * T, G = 4 * R;
  // every g_* may be NULL (a frozen weight): its GEMM / column sum is skipped, and so is the part of the chain that reaches no
  // gradient (the layers below the lowest one with a weight to train, the embedding's input gradient)
  bool below[4];                                       // a gradient is wanted at layer l or under it (embedding included)
  for (int l = 0; l < NL; ++l) {
    bool has = false;
    for (int dr = 0; dr < 2; ++dr) has = has || a->g_w_ih[l][dr] || a->g_w_hh[l][dr] || a->g_b_ih[l][dr] || a->g_b_hh[l][dr];
    below[l] = has || (l == 0 ? a->g_emb != nullptr : below[l - 1]);
  }
  const bool need_proj = a->g_w_proj || a->g_b_proj || below[NL - 1];
  // ---- srl_arg_words_out_enc
  const int MA = Bn * nsrl;
  lin_dpre(a->d_lang_enc, L, 1, b.lenc, 1, b.dpre, MA, L, st);
  if (a->g_w_arg) VOG_TRY(gemm_f32(b.dpre, 1, L, b.enc, 2 * D, 1, a->g_w_arg, 2 * D, nullptr, 0, L, 2 * D, MA, st));
  if (a->g_b_arg) VOG_TRY(colsum(b.dpre, a->g_b_arg, b.part, MA, L, st));
  if (!need_proj) { VOG_LAUNCH_CHECK(); return 0; }
  VOG_TRY(gemm_f32(b.dpre, L, 1, a->w_arg, 2 * D, 1, b.denc, 2 * D, nullptr, 0, MA, 2 * D, L, st));
  ::vog::launch(argvec_scatter_kernel, blocks((int64_t)BT * D), dim3(256), 0, st, (const float*)b.denc, a->capture, b.dfull, Bn, nsrl, T, D);
  // ---- lstm_out_feat_proj, the per-step call
  lin_dpre(b.dfull, D, 1, b.full, 1, b.dpre2, BT, D, st);
  if (a->g_w_proj) VOG_TRY(gemm_f32(b.dpre2, 1, D, b.lout[NL - 1], 2 * R, 1, a->g_w_proj, 2 * R, nullptr, 0, D, 2 * R, BT, st));
  if (a->g_b_proj) VOG_TRY(colsum(b.dpre2, a->g_b_proj, b.part, BT, D, st));
  // ---- ... and the call on final_hidden (d_hid: the gradient of the sep verb head's feature): final_hidden = the top layer's
  // state slot T of both directions (the forward direction's state after step len-1, the reverse one's after position 0)
  if (a->d_hid) {
    concat_rows(b.hst[NL - 1][0] + (int64_t)T * Bn * R, R, 1, b.hst[NL - 1][1] + (int64_t)T * Bn * R, R, 1, b.hfin, Bn, st);
    VOG_TRY(gemm_f32(b.hfin, 2 * R, 1, a->w_proj, 1, 2 * R, b.hpre, D, a->b_proj, 1, Bn, D, 2 * R, st));      // hid (its ReLU mask)
    lin_dpre(a->d_hid, D, 1, b.hpre, 1, b.dpreh, Bn, D, st);
    if (a->g_w_proj) VOG_TRY(gemm_f32(b.dpreh, 1, D, b.hfin, 2 * R, 1, a->g_w_proj, 2 * R, nullptr, 0, D, 2 * R, Bn, st, 1));   // +=
    if (a->g_b_proj) {
      VOG_TRY(colsum(b.dpreh, b.hpre, b.part, Bn, D, st));                                             // (hpre is free again)
      ::vog::launch(vec_add_kernel, blocks(D), dim3(256), 0, st, (const float*)a->g_b_proj, (const float*)b.hpre, a->g_b_proj, D);
    }
    VOG_TRY(gemm_f32(b.dpreh, D, 1, a->w_proj, 2 * R, 1, b.dfin, 2 * R, nullptr, 0, Bn, 2 * R, D, st));     // d final_hidden
  }
  if (!below[NL - 1]) { VOG_LAUNCH_CHECK(); return 0; }
  float* d_out = b.dxa; float* d_in = b.dxb;
  VOG_TRY(gemm_f32(b.dpre2, D, 1, a->w_proj, 2 * R, 1, d_out, 2 * R, nullptr, 0, BT, 2 * R, D, st));
  // ---- BiLSTM, top layer first, down to the lowest layer with a gradient to produce
  for (int l = NL - 1; l >= 0 && below[l]; --l) {
    const float* xin = l == 0 ? b.x0 : b.lout[l - 1];
    const int K = l == 0 ? E : 2 * R;
    const bool want_dx = l == 0 ? a->g_emb != nullptr : below[l - 1];
    const Drop dl = make_drop(a->drop_out, a->drop_seed, l < NL - 1 ? 2 + l : 10);
    if (dl.thr) mask_mul(d_out, d_out, dl, (int64_t)BT * 2 * R, st);
    // the weight and input gradients of one direction from its dG by step / by position
    auto dir_grads = [&](int dr, const float* dGs_, const float* dGp_) -> int {
      if (a->g_w_hh[l][dr])                                                                                      // sum_s dG_s^T h_{s-1}
        VOG_TRY(gemm_f32(dGs_, 1, G, b.hst[l][dr], R, 1, a->g_w_hh[l][dr], R, nullptr, 0, G, R, BT, st));
      if (a->g_w_ih[l][dr]) VOG_TRY(gemm_f32(dGp_, 1, G, xin, K, 1, a->g_w_ih[l][dr], K, nullptr, 0, G, K, BT, st));   // dG^T x
      float* gb = a->g_b_ih[l][dr] ? a->g_b_ih[l][dr] : a->g_b_hh[l][dr];
      if (gb) VOG_TRY(colsum(dGp_, gb, b.part, BT, G, st));
      if (a->g_b_ih[l][dr] && a->g_b_hh[l][dr])
        VOG_TRY(dev_copy(a->g_b_hh[l][dr], a->g_b_ih[l][dr], (size_t)G * 4, st));
      if (want_dx) VOG_TRY(gemm_f32(dGp_, G, 1, a->w_ih[l][dr], K, 1, d_in, K, nullptr, 0, BT, K, G, st, dr));     // d x (both directions)
      return 0;
    };
    if (amp || fused) {                                // both directions at once, from W_hh^T of both: amp's wt16, or in fp32
      LstmRecur r = lstm_recur_args(a, b, l);          // transposed here once per layer (carved rows of 4R floats: wvec = 1)
      float* const wt[2] = {b.whh_t, b.whh_t1};
      for (int dr = 0; dr < 2; ++dr) {
        VOG_TRY(lang_bwd_dir_init(a, b, l, dr, r.dGp[dr], r.dh[dr], r.dc[dr], st));
        if (!amp) transpose_f32(a->w_hh[l][dr], wt[dr], G, R, st);               // [R, 4R]
        r.w[dr] = amp ? (const void*)b.wt16[l][dr] : wt[dr];
      }
      r.d_out = d_out;
      r.wvec = amp ? (G & 7) == 0 && al16(r.w[0]) && al16(r.w[1]) : 1;
      for (int t = T - 1; t >= 0; --t) {
        r.s = t; r.first = t == T - 1;
        lstm_recur_launch(r, amp, split, true, st);
      }
      for (int dr = 0; dr < 2; ++dr) VOG_TRY(dir_grads(dr, r.dGs[dr], r.dGp[dr]));
    } else {
      for (int dr = 0; dr < 2; ++dr) {
        VOG_TRY(lang_bwd_dir_init(a, b, l, dr, b.dGp, b.dh0, b.dc, st));
        float *cur = b.dh0, *nxt = b.dh1;
        transpose_f32(a->w_hh[l][dr], b.whh_t, G, R, st);                        // [R, 4R]
        for (int t = T - 1; t >= 0; --t) {
          LstmStep ls{}; ls.lens = a->lens; ls.gates = b.gates[l][dr]; ls.c = b.cst[l][dr]; ls.h = b.hst[l][dr]; ls.Bn = Bn; ls.T = T; ls.R = R;
          ls.s = t; ls.reverse = dr; ls.d_out = d_out; ls.dh_cur = cur; ls.dh_nxt = nxt; ls.dc = b.dc; ls.dGs = b.dGs; ls.dGp = b.dGp;
          ::vog::launch(lstm_cell_bwd_kernel, blocks((int64_t)Bn * R), dim3(256), 0, st, ls);
          // dh_{s-1} += dG_s W_hh
          VOG_TRY(gemm_f32(b.dGs + (int64_t)t * Bn * G, G, 1, b.whh_t, 1, G, nxt, R, nullptr, 0, Bn, R, G, st, 1));
          float* sw = cur; cur = nxt; nxt = sw;
        }
        VOG_TRY(dir_grads(dr, b.dGs, b.dGp));
      }
    }
    float* sw = d_out; d_out = d_in; d_in = sw;
  }
  if (a->g_emb) {
    const Drop drop_emb = make_drop(a->drop_in, a->drop_seed, 1);
    if (drop_emb.thr) mask_mul(d_out, d_out, drop_emb, (int64_t)BT * E, st);
    const int nv = a->vocab_size + 1;
    ::vog::launch(embed_scatter_kernel, blocks((int64_t)nv * E), dim3(256), 0, st, (const float*)d_out, (const int64_t*)b.tok, a->g_emb, BT, E, nv);
  }
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_lang_f32(const vog_lang_f32_args* a, void* stream) {
  VOG_CHECK_ARG(a && a->words_ind && a->word_mask && a->lens && a->capture && a->emb && a->w_proj && a->b_proj && a->w_arg && a->b_arg);
  VOG_CHECK_ARG(a->Bn > 0 && a->T > 0 && a->nsrl > 0 && a->E > 0 && a->R > 0 && a->layers > 0 && a->layers <= 4 && a->D > 0 && a->L > 0);
  VOG_CHECK_ARG(a->T <= a->mask_len && a->scratch);
  if ((int64_t)a->scratch_bytes < vog_lang_f32_scratch_bytes(a->Bn, a->T, a->nsrl, a->E, a->R, a->layers, a->D, a->L))
    VOG_FAIL(-2, "vog_lang_f32: scratch too small");
  for (int l = 0; l < a->layers; ++l)
    for (int dr = 0; dr < 2; ++dr) VOG_CHECK_ARG(a->w_ih[l][dr] && a->w_hh[l][dr] && a->b_ih[l][dr] && a->b_hh[l][dr]);
  const bool bwd = a->d_lang_enc != nullptr;
  const int amp = train_amp();                                    // (the scratch size above follows the same switches)
  const int fused = amp ? 0 : train_int(TRAIN_LSTM_FUSED);        // amp keeps its own fused recurrence
  const int split = amp ? train_int(TRAIN_LSTM_AMP_SPLIT) : 0;    // ... in its tile form or, with "lstm_amp_split", with K split over waves
  hipStream_t st = (hipStream_t)stream;
  const int R = a->R, G = 4 * R, NL = a->layers;
  const LangBufs b = lang_layout(a->scratch, a->Bn, a->T, a->nsrl, a->E, R, NL, a->D, a->L, amp, fused);
  // amp: the 16-bit recurrent weights (one conversion launch per call: w16 for the forward, wt16 for the backward)
  if (amp) {
    Whh16 cv{};
    cv.G = G; cv.R = R;
    for (int l = 0; l < NL; ++l)
      for (int dr = 0; dr < 2; ++dr) {
        cv.w[l * 2 + dr] = a->w_hh[l][dr];
        cv.w16[l * 2 + dr] = a->reuse_forward ? nullptr : b.w16[l][dr];
        cv.wt16[l * 2 + dr] = bwd ? b.wt16[l][dr] : nullptr;
      }
    amp_type(amp, [&](auto ty) {
      ::vog::launch(whh16_kernel<decltype(ty)>, dim3(ceil_div(R, 32), ceil_div(G, 32), NL * 2), dim3(256), 0, st, cv);
    });
  }
  // reuse_forward: `scratch` still holds the forward of an earlier call with the same inputs, weights and dropout seed
  // (the trainer's forward pass): the backward starts from it instead of recomputing 2 T recurrent products per layer
  if (!a->reuse_forward) VOG_TRY(lang_forward(a, b, amp, fused, split, st));
  if (!bwd) { VOG_LAUNCH_CHECK(); return 0; }
  return lang_backward(a, b, amp, fused, split, st);
}
