// Device weight packers: every weight image vog_ctx_finalize builds on the host (casts, hi + lo remainders, head padding,
// 16x32 / 32x16 fragment order, BiLSTM tiles, [W_fwd ; W_bwd], b_ih + b_hh, the gate table's operands), written in place
// from fp32 DEVICE sources (vog_ctx_refresh_device, forward.hip). Placement comes from the index maps of wpack_dev.h, the
// same functions the host packers call; the roundings are the host's for finite values (wpack_dev.h).
//
// One thread per destination group of 8 elements (16 bytes of halves). In every layout that group is 8 consecutive columns
// of one row of the image's view, so where the 8 sources are contiguous and 16-byte aligned the thread moves two 16-byte
// loads into one 16-byte store; elsewhere (head slices of 171 / 171 / 170 rows or columns, partial padding, flat tails) it
// goes element by element and leaves padding alone. No thread stores at or past the image's byte count.
#include <type_traits>
#include "wpack_dev.h"

namespace vog {

template <typename T16>
__device__ __forceinline__ unsigned short wpack_cvt(float w, int lo) {
  if (lo) w = w - from16<T16>(to16<T16>(w));       // exact in fp32; then the same rounding
  return to16<T16>(w);
}

// DT: 0 bf16, 1 f16, 2 fp32
template <int DT>
__global__ __launch_bounds__(256) void wpack_kernel(WpackImage m) {
  using T16 = typename std::conditional<DT == 0, BF16, F16>::type;
  constexpr int ESZ = DT == 2 ? 4 : 2;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= wpack_groups(m)) return;
  int n, k;
  wpack_layout_src(m.layout, g, m.K, m.R, &n, &k);
  const int64_t left = (int64_t)m.N * m.K - g * 8;       // (only a flat plain image ends inside a group)
  const int cnt = left < 8 ? (int)left : 8;
  const int64_t off = g * 8 * ESZ;
  if (off + (int64_t)cnt * ESZ > m.bytes) return;
  char* dst = (char*)m.dst + off;

  if (m.view == WV_BIAS || m.view == WV_GATE_BIAS) {      // b_ih + b_hh: one fp32 add
    for (int j = 0; j < cnt; ++j) {
      int which;
      const int64_t o = wpack_view_src(m, n, k + j, &which);
      ((float*)dst)[j] = m.src[2 * which][o] + m.src[2 * which + 1][o];
    }
    return;
  }

  int w0, w1;
  const int64_t o0 = wpack_view_src(m, n, k, &w0), o1 = wpack_view_src(m, n, k + cnt - 1, &w1);
  // first and last present, 7 apart, in one source: every view is monotone along a row, so all 8 are contiguous
  const float* p0 = o0 >= 0 ? m.src[w0] + o0 : nullptr;
  if (cnt == 8 && o0 >= 0 && o1 == o0 + 7 && w0 == w1 && ((uintptr_t)p0 & 15) == 0 && ((uintptr_t)dst & 15) == 0) {
    const f32x4 a = *(const f32x4*)p0, b = *(const f32x4*)(p0 + 4);
    if (DT == 2) {
      ((f32x4*)dst)[0] = a; ((f32x4*)dst)[1] = b;
    } else {
      u16x8 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) { r[j] = wpack_cvt<T16>(a[j], m.lo); r[4 + j] = wpack_cvt<T16>(b[j], m.lo); }
      *(u16x8*)dst = r;
    }
    return;
  }
  for (int j = 0; j < cnt; ++j) {
    int which;
    const int64_t o = wpack_view_src(m, n, k + j, &which);
    if (o < 0) continue;                                  // padding keeps finalize's zero
    const float w = m.src[which][o];
    if (DT == 2) ((float*)dst)[j] = w;
    else ((unsigned short*)dst)[j] = wpack_cvt<T16>(w, m.lo);
  }
}

int wpack_launch(const WpackImage& m, hipStream_t st) {
  VOG_CHECK_ARG(m.dst && m.bytes > 0 && m.N > 0 && m.K > 0 && m.src[0]);
  VOG_CHECK_ARG(m.dt >= -1 && m.dt <= 1 && (m.dt >= 0 || !m.lo));
  VOG_CHECK_ARG((m.K % 8) == 0 || (m.N == 1 && m.layout == WL_PLAIN));
  VOG_CHECK_ARG(m.layout != WL_FRAG16 || ((m.N % 16) == 0 && (m.K % 32) == 0));
  VOG_CHECK_ARG(m.layout != WL_FRAG32 || ((m.N % 32) == 0 && (m.K % 16) == 0));
  VOG_CHECK_ARG(m.layout != WL_LSTM || (m.R > 0 && (m.R % 4) == 0 && (m.K % 32) == 0 && m.N == 8 * m.R));
  VOG_CHECK_ARG((int64_t)m.N * m.K * (m.dt < 0 ? 4 : 2) <= m.bytes);
  const int64_t groups = wpack_groups(m);
  VOG_CHECK_ARG(groups < (int64_t)1 << 38);
  const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
  if (m.dt == VOG_BF16) launch(wpack_kernel<0>, grid, block, 0, st, m);
  else if (m.dt == VOG_F16) launch(wpack_kernel<1>, grid, block, 0, st, m);
  else launch(wpack_kernel<2>, grid, block, 0, st, m);
  VOG_LAUNCH_CHECK();
  return 0;
}

}  // namespace vog

// Host only: out[i] = linear index, in the row-major source, of the element a packer places at destination position i.
// layout 1: vog_pack_w_frag of [N, K]; 2: vog_pack_w_frag32 of [N, K]; 3: vog_lstm_pack_w with R = N, source [W_fwd ; W_bwd]
// = [8R, K], destination 8 * R * K elements.
extern "C" int vog_wpack_index_map(int layout, int N, int K, int64_t* out) {
  VOG_CHECK_ARG(out && N > 0 && K > 0);
  VOG_CHECK_ARG(layout == vog::WL_FRAG16 || layout == vog::WL_FRAG32 || layout == vog::WL_LSTM);
  VOG_CHECK_ARG(layout != vog::WL_FRAG16 || ((N % 16) == 0 && (K % 32) == 0));
  VOG_CHECK_ARG(layout != vog::WL_FRAG32 || ((N % 32) == 0 && (K % 16) == 0));
  VOG_CHECK_ARG(layout != vog::WL_LSTM || ((N % 4) == 0 && (K % 32) == 0));
  const int64_t total = (int64_t)(layout == vog::WL_LSTM ? 8 * N : N) * K;
  for (int64_t g = 0; g < total / 8; ++g) {
    int n, k;
    vog::wpack_layout_src(layout, g, K, N, &n, &k);
    for (int j = 0; j < 8; ++j) out[g * 8 + j] = (int64_t)n * K + k + j;
  }
  return 0;
}
