// Weight images: where every element of a derived device weight buffer comes from. One body per layout, called by the host
// packers (vog_pack_w_frag, vog_pack_w_frag32, vog_lstm_pack_w, the padded gathers of finalize_tx) and by the device pack
// kernels (wpack.hip), so that the two sides cannot place an element differently.
//
// An image is a LAYOUT over a VIEW. The view is a logical fp32 matrix [N, K] whose elements are elements of the source weights
// (or padding, which nobody writes: it holds the zeros vog_ctx_finalize put there). The layout says which 8 consecutive columns
// of which row of that matrix make up destination group g (8 elements: 16 bytes of halves, what one lane loads).
//
// Rounding: f16 is the plain _Float16 conversion, bf16 rounds to nearest even. The host's bf16 bit arithmetic and the hardware
// conversion the device uses differ only for NaN inputs; NaN weights are out of scope for the device path.
#pragma once
#include "common.h"

namespace vog {

enum WpackLayout { WL_PLAIN = 0, WL_FRAG16 = 1, WL_FRAG32 = 2, WL_LSTM = 3 };
enum WpackView {
  WV_DIRECT = 0,      // M[n, k] = src0[n * ld + k0 + k]
  WV_QKV = 1,         // rows of the head-padded [3 * H * dp, .] Wq / Wk / Wv: M[n, k] = src[which][head_src(n) * ld + k0 + k]
  WV_WO = 2,          // columns of the head-padded [d, H * dp] Wo: M[n, k] = src0[n * ld + head_src(k)]
  WV_CAT = 3,         // both directions under each other: M[n, k] = src[n / (4R)][(n % 4R) * K + k]
  WV_GATE = 4,        // gate-table order, row (dir, unit, gate) = src[dir][(gate * R + unit) * K + k]
  WV_BIAS = 5,        // [1, 8R]: b_ih + b_hh, src[2 * dir] + src[2 * dir + 1]
  WV_GATE_BIAS = 6    // the same sums in gate-table order
};

struct WpackImage {
  void* dst;
  int64_t bytes;            // of the image: nothing is stored at or past dst + bytes
  const float* src[4];
  int layout, view;
  int dt;                   // vog_dtype of the destination, -1: fp32
  int lo;                   // remainder image: t16(w - back(t16(w)))
  int N, K;                 // the logical matrix
  int64_t ld;               // source row stride (elements)
  int k0;                   // first source column
  int H, dp, chunk, d;      // head geometry (torch.chunk: heads of `chunk` rows, the last one shorter), padded to dp each
  int R;
};

// position p of a head-padded axis [H * dp] -> index on the unpadded axis [d], -1 for padding
__host__ __device__ inline int wpack_head_src(int p, int H, int dp, int chunk, int d) {
  const int h = p / dp, dd = p % dp, off = h * chunk;
  const int sz = d - off < chunk ? d - off : chunk;
  return (h < H && dd < sz) ? off + dd : -1;
}

// ---- layouts: destination group g -> (row, first of 8 columns) ---------------------------------------------------------
// 16x32 fragments (vog_pack_w_frag): [N/16][K/32][64 lanes][8], lane l holds row l & 15, columns (l >> 4) * 8 ...
__host__ __device__ inline void wpack_frag16_src(int64_t g, int K, int* n, int* k) {
  const int ksteps = K >> 5, lane = (int)(g & 63);
  const int64_t t = g >> 6;
  *n = (int)(t / ksteps) * 16 + (lane & 15);
  *k = (int)(t % ksteps) * 32 + (lane >> 4) * 8;
}
// 32x16 fragments (vog_pack_w_frag32): [N/32][K/16][64 lanes][8], lane l holds row l & 31, columns (l >> 5) * 8 ...
__host__ __device__ inline void wpack_frag32_src(int64_t g, int K, int* n, int* k) {
  const int ks_n = K >> 4, lane = (int)(g & 63);
  const int64_t t = g >> 6;
  *n = (int)(t / ks_n) * 32 + (lane & 31);
  *k = (int)(t % ks_n) * 16 + (lane >> 5) * 8;
}
// BiLSTM tiles (vog_lstm_pack_w): [dir][R/4][K/32][64 lanes][8]; tile row = unit_local * 4 + gate. The row returned is the
// row of [W_fwd ; W_bwd] ([8R, K]): dir * 4R + gate * R + unit.
__host__ __device__ inline void wpack_lstm_src(int64_t g, int R, int K, int* n, int* k) {
  const int ksteps = K >> 5, lane = (int)(g & 63), rr = lane & 15;
  int64_t t = g >> 6;
  const int ks = (int)(t % ksteps); t /= ksteps;
  const int tile = (int)(t % (R / 4)), dir = (int)(t / (R / 4));
  *n = dir * 4 * R + (rr & 3) * R + tile * 4 + (rr >> 2);
  *k = ks * 32 + (lane >> 4) * 8;
}
// row-major; a matrix whose K is no multiple of 8 is taken flat (N = 1)
__host__ __device__ inline void wpack_plain_src(int64_t g, int K, int* n, int* k) {
  const int64_t e = g * 8;
  *n = (int)(e / K);
  *k = (int)(e % K);
}

__host__ __device__ inline void wpack_layout_src(int layout, int64_t g, int K, int R, int* n, int* k) {
  if (layout == WL_FRAG16) wpack_frag16_src(g, K, n, k);
  else if (layout == WL_FRAG32) wpack_frag32_src(g, K, n, k);
  else if (layout == WL_LSTM) wpack_lstm_src(g, R, K, n, k);
  else wpack_plain_src(g, K, n, k);
}

// ---- views: element (n, k) of the logical matrix -> offset into source `*which`, -1 for padding -------------------------
__host__ __device__ inline int64_t wpack_view_src(const WpackImage& m, int n, int k, int* which) {
  *which = 0;
  switch (m.view) {
    case WV_QKV: {
      const int hp = m.H * m.dp, r = wpack_head_src(n % hp, m.H, m.dp, m.chunk, m.d);
      *which = n / hp;
      return r < 0 ? -1 : (int64_t)r * m.ld + m.k0 + k;
    }
    case WV_WO: {
      const int cc = wpack_head_src(k, m.H, m.dp, m.chunk, m.d);
      return cc < 0 ? -1 : (int64_t)n * m.ld + cc;
    }
    case WV_CAT:
      *which = n / (4 * m.R);
      return (int64_t)(n % (4 * m.R)) * m.K + k;
    case WV_GATE: {
      const int q = n % (4 * m.R), u = q >> 2, gate = q & 3;
      *which = n / (4 * m.R);
      return (int64_t)(gate * m.R + u) * m.K + k;
    }
    case WV_BIAS:
      *which = k / (4 * m.R);
      return k % (4 * m.R);
    case WV_GATE_BIAS: {
      const int q = k % (4 * m.R), u = q >> 2, gate = q & 3;
      *which = k / (4 * m.R);
      return gate * m.R + u;
    }
    default:
      return (int64_t)n * m.ld + m.k0 + k;
  }
}

// number of 8-element destination groups of an image
__host__ __device__ inline int64_t wpack_groups(const WpackImage& m) { return ((int64_t)m.N * m.K + 7) / 8; }

int wpack_launch(const WpackImage& img, hipStream_t st);

}  // namespace vog
