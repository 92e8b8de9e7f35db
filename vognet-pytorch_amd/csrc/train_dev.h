// What the four training sources (train_gemm.hip, train_tx.hip, train_attn.hip, train_lang.hip) share: the dropout generator, the scratch
// carve, two device one-liners, and the host helpers one file offers the others. A kernel is defined in exactly one file; the
// others reach it through these launchers.
#pragma once
#include "common.h"

namespace vog {

// ---- train-mode dropout: counter-based masks, recomputed wherever they are needed (forward, backward): element idx of
// site `site` is kept iff the top 32 bits of splitmix64(seed * 0x9E3779B97F4A7C15 + site * 0xBF58476D1CE4E5B9 + idx)
// are >= p * 2^32; kept elements are scaled by 1 / (1 - p). The CPU oracle restates it (oracle/vog_oracle.py::drop_mask).
// `tick` (NULL = the seed is the host's, as always): the iteration count of a captured step in device memory (vog_train_step,
// csrc/train_step.hip); `seed` is then the seed's base and the masks are those of seed (base + *tick) & (2^63 - 1) - what the
// host hands over for that iteration, so a replayed launch draws a new mask every step.
struct Drop { unsigned long long seed; unsigned int site; unsigned int thr; float inv_keep; const unsigned long long* tick; };   // thr == 0: off
__device__ __forceinline__ float drop_scale(const Drop& d, unsigned long long idx) {
  if (d.thr == 0) return 1.0f;
  const unsigned long long seed = d.tick ? ((d.seed + *d.tick) & 0x7FFFFFFFFFFFFFFFull) : d.seed;
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull + (unsigned long long)d.site * 0xBF58476D1CE4E5B9ull + idx;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned int)(z >> 32) >= d.thr ? d.inv_keep : 0.0f;
}
Drop make_drop(float p, unsigned long long seed, int site);
void mask_mul(const float* in, float* out, const Drop& d, int64_t n, hipStream_t st);            // out[i] = in[i] * mask(i)   (train_tx.hip)

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- products (train_gemm.hip): C = A . B (+ bias, relu, accumulate) with generic strides, operand type by the calling thread's
// switches; the batched form; out[n, k] = in[k, n]; the calling thread's "amp" switch (0 | 1 bf16 | 2 f16)
int gemm_f32_b(const float* a, int64_t am, int64_t ak, int64_t sa, const float* b, int64_t bk, int64_t bn, int64_t sb,
               float* c, int64_t ldc, int64_t sc, const float* bias, int relu, int accum, int M, int N, int K, int batch,
               hipStream_t st);
int gemm_f32(const float* a, int64_t am, int64_t ak, const float* b, int64_t bk, int64_t bn, float* c, int64_t ldc,
             const float* bias, int relu, int M, int N, int K, hipStream_t st, int accum = 0);
void transpose_f32(const float* in, float* out, int rows, int cols, hipStream_t st);
// The calling thread's switches and launch counters, in the order of the one table that vog_train_set_int / vog_train_get_int
// walk (train_gemm.hip: names, ranges and what each one means). A counter is bumped by whoever launches: ++train_int(...).
enum TrainInt { TRAIN_BF16_GEMM, TRAIN_AMP, TRAIN_F32_PRODUCTS, TRAIN_LSTM_FUSED, TRAIN_LSTM_FUSED_LAUNCHES, TRAIN_LSTM_AMP_SPLIT,
                TRAIN_LSTM_AMP_SPLIT_LAUNCHES, TRAIN_GEMM_AMP_PIPE, TRAIN_GEMM_AMP_PIPE_LAUNCHES, TRAIN_ATTN_FUSED_PIPE,
                TRAIN_ATTN_FUSED_PIPE_LAUNCHES, TRAIN_ATTN_VL_LAUNCHES, TRAIN_KERNEL_FILLS, TRAIN_INTS };
int& train_int(TrainInt i);
// The calling thread's pointer switches (vog_train_set_ptr, beside the integers): "drop_tick" = the device iteration count that
// make_drop hands to every Drop it builds (NULL, the default: none).
enum TrainPtr { TRAIN_DROP_TICK, TRAIN_PTRS };
const void*& train_ptr(TrainPtr i);
// Device fills and copies of the training path (train_gemm.hip): hipMemsetAsync / hipMemcpyAsync / hipMemcpy2DAsync as always -
// but with the calling thread's "kernel_fills" switch on (a trainer sets it while it records a captured step) they are KERNELS,
// so that the graph is one chain of kernel nodes and holds no memset or memcpy node. Sizes and pitches are multiples of 4 bytes.
int dev_zero(void* p, size_t bytes, hipStream_t st);
int dev_copy(void* dst, const void* src, size_t bytes, hipStream_t st);
int dev_copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipStream_t st);
inline int train_amp() { return train_int(TRAIN_AMP); }
inline void count_f32_product() { ++train_int(TRAIN_F32_PRODUCTS); }   // one more launch of an fp32 product kernel by this thread
// the run-time "amp" value (1 | 2) as a type tag: f(BF16{}) | f(F16{})
template <typename F> void amp_type(int amp, F&& f) { if (amp == 1) f(BF16{}); else f(F16{}); }

// ---- column sums (train_tx.hip): out[n] = sum_m in[m, n] through CS_CHUNKS rows of partials
constexpr int CS_CHUNKS = 64;
struct ColPart { float* p; int width; };          // the partials: CS_CHUNKS rows of `width` floats
int colsum(const float* in, float* out, const ColPart& part, int M, int d, hipStream_t st);

// ---- caller-owned scratch: every operator has ONE layout function that walks a Carve - on no base for its *_scratch_bytes
// (only counts), on the caller's pointer for the entry - so the size it declares is the end of its last carve (`bytes`).
// A carve advances by its bytes rounded up to pad_floats floats; align_base_256 starts at the next 256-byte boundary and
// counts the worst case, 255 bytes, for it. No kernel reads past the end of an operator's last carve (the column sums, the
// pe_* store, lin_dpre_kernel, the GEMM tiles and the LSTM cells all index by row and column): nothing lies behind bytes().
struct Carve {
  int64_t lead, pad, off = 0; char* base;
  Carve(void* b, int pad_floats, bool align_base_256)
      : lead(align_base_256 ? 255 : 0), pad(pad_floats * 4), base((char*)(((uintptr_t)b + lead) & ~(uintptr_t)lead)) {}
  template <typename T> T* take(int64_t count) {       // count in units of T
    T* r = base ? (T*)(base + off) : nullptr;
    off += (count * (int64_t)sizeof(T) + pad - 1) / pad * pad;
    return r;
  }
  ColPart colpart(int width) { return ColPart{take<float>((int64_t)CS_CHUNKS * width), width}; }
  int64_t bytes() const { return lead + off; }          // from the caller's pointer
};

// ---- row pieces (train_tx.hip): dpre[m, n] = [y > 0] * sum_{j < rep} dy[(m*rep + j) * ldy + n]; out[m] = [a[m / rep_a] | b[m / rep_b]]
void lin_dpre(const float* dy, int64_t ldy, int rep, const float* y, int relu, float* dpre, int M, int N, hipStream_t st);
void concat_rows(const float* a, int Na, int rep_a, const float* b, int Nb, int rep_b, float* out, int M, hipStream_t st);
// bx[r] = (x1/w, y1/h, x2/w, y2/h, frame/fdiv, 0, 0, 0): the normalised boxes of the attention bias, 8 floats per proposal row
void norm_boxes(const float* props, int stride, float vw, float vh, float fdiv, float* bx, int rows, hipStream_t st);

// ---- the attention operators on the factors of mul_tx's layer-0 input (train_tx.hip; vog_attn_vl, include/vog_hip.h):
// vl_check: the descriptor against the operator's geometry - argument errors, then -2 for a short scratch, no device call;
// vl_forward: q, k, v [S*N, d] from the factors; vl_backward: everything behind dq / dk / dv (the weight gradients into g_w*,
// NULL = not wanted; d_ps / d_lang of the descriptor). dq / dk / dv are read only where an output needs them.
int vl_check(const vog_attn_vl* vl, const float* d_x, int S, int N, int n, int d);
int vl_forward(const vog_attn_vl* vl, const float* wq, const float* wk, const float* wv, float* q, float* k, float* v, int n,
               hipStream_t st);
int vl_backward(const vog_attn_vl* vl, const float* wq, const float* wk, const float* wv, const float* dq, const float* dk,
                const float* dv, float* g_wq, float* g_wk, float* g_wv, int n, hipStream_t st);

}  // namespace vog
