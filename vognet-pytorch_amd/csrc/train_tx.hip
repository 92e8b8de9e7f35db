// The row-wise and element-wise side of the fp32 / mixed-precision training path, forward and backward: dropout masks, LayerNorm,
// column sums, attention rows and box terms, the concatenations, and the entries of the encoder-layer tail, attention, Linear and
// score head; Adam. Its products are train_gemm.hip's, the language side is train_lang.hip.
//
// SURVEY.md 8(f)-4, first slice of the backward: from d loss / d mdl_outs (vog_loss_bwd) through the score head
// (lin2: code/mdl_vog.py:224-230) and the tail of the LAST mul_tx encoder layer - Wo, residual, LayerNorm,
// FFN, residual, LayerNorm (code/transformer_code.py:21-31, 73-81, 189-203) - to the gradients of every
// parameter on that path and of the tail's two inputs (the concatenated attention heads and the layer
// input). What the reference gets from autograd in Learner.train_epoch (utils/trn_utils.py:485-532).
//
// fp32 throughout, on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32: exact fp32 products and sums, 1/16 of
// the 16-bit MFMA rate): this slice pins the MATH against autograd through the reference modules
// (tests/golden/bwd__*.npz); the 16-bit operand path of the forward kernels is the next step. The forward
// tail keeps its fp32 stream in registers and writes nothing back, so the backward recomputes the
// activations it needs from the tail's inputs (activation recomputation, fp32).
//
//   t = a Wo^T + x            x1 = LN1(t)
//   f = relu(x1 W1^T + b1)    u = f W2^T + b2 + x1      y = LN2(u)
//   h = relu(y Wl^T + bl)     logit = h . w2 + b2'      mdl_outs[v, arg, frame*nppf + p] = logit(row)
#include <algorithm>
#include "train_dev.h"

namespace vog {

Drop make_drop(float p, unsigned long long seed, int site) {
  // (the calling thread's "drop_tick" pointer, vog_train_set_ptr: with it `seed` is the base of a device-counted seed)
  Drop d{seed, (unsigned int)site, 0u, 1.0f, (const unsigned long long*)train_ptr(TRAIN_DROP_TICK)};
  if (p > 0.f) {
    const double pd = (double)p;
    d.thr = (unsigned int)(unsigned long long)(pd * 4294967296.0);
    d.inv_keep = (float)(1.0 / (1.0 - pd));
  }
  return d;
}
// out[i] = in[i] * mask(i)
__global__ void mask_mul_kernel(const float* in, float* out, Drop d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] * drop_scale(d, (unsigned long long)i);
}
void mask_mul(const float* in, float* out, const Drop& d, int64_t n, hipStream_t st) {
  ::vog::launch(mask_mul_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, d, n);
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- row-wise pieces -----------------------------------------------------------------------------
// t = t + x (optional), stats[m] = (mean, rstd), y = (t - mean) * rstd * g + b      one wave per row
__global__ __launch_bounds__(256) void ln_fwd_kernel(float* t, const float* x, const float* g, const float* b, float* y,
                                                     float2* stats, int M, int d, Drop dr) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  float* tr = t + (int64_t)row * d;
  float s = 0.f;
  for (int i = lane; i < d; i += 64) {        // t = dropout(t) + x  (ResidualBlock: x + dropout(layer(x)))
    float v = tr[i];
    if (x) { v = v * drop_scale(dr, (unsigned long long)row * d + i) + x[(int64_t)row * d + i]; tr[i] = v; }
    s += v;
  }
  const float mean = wsum(s) / (float)d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) { const float c = tr[i] - mean; q += c * c; }
  const float rstd = 1.0f / sqrtf(wsum(q) / (float)d + 1e-5f);
  for (int i = lane; i < d; i += 64) y[(int64_t)row * d + i] = (tr[i] - mean) * rstd * g[i] + b[i];
  if (lane == 0) stats[row] = make_float2(mean, rstd);
}

// dt = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)), dxh = dy * g, xh = (t - mean) * rstd; also writes
// dyxh = dy * xh (the summand of d gamma). `add` (optional) is added to dy first (a second gradient path).
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* dy, const float* add, const float* t, const float2* stats,
                                                     const float* g, float* dt, float* dyxh, float* dysum, int M, int d) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float2 st = stats[row];
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < d; i += 64) {
    const int64_t o = (int64_t)row * d + i;
    const float dv = dy[o] + (add ? add[o] : 0.f);
    const float xh = (t[o] - st.x) * st.y, dxh = dv * g[i];
    s1 += dxh; s2 += dxh * xh;
    dyxh[o] = dv * xh;
    if (dysum) dysum[o] = dv;
  }
  s1 = wsum(s1) / (float)d; s2 = wsum(s2) / (float)d;
  for (int i = lane; i < d; i += 64) {
    const int64_t o = (int64_t)row * d + i;
    const float dv = dy[o] + (add ? add[o] : 0.f);
    const float xh = (t[o] - st.x) * st.y;
    dt[o] = st.y * (dv * g[i] - s1 - xh * s2);
  }
}

// out[n] = sum_m in[m, n] in two fixed-order levels (reproducible): CS_CHUNKS row chunks x 64-column blocks write
// partial sums, then one thread per column adds the chunks in order.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* in, float* part, int M, int d) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, n = blockIdx.x * 64 + lane;
  const int rows = (M + CS_CHUNKS - 1) / CS_CHUNKS, r0 = blockIdx.y * rows, r1 = min(M, r0 + rows);
  float s = 0.f;
  if (n < d) for (int m = r0 + wid; m < r1; m += 4) s += in[(int64_t)m * d + n];
  red[wid][lane] = s;
  __syncthreads();
  if (wid == 0 && n < d) part[(int64_t)blockIdx.y * d + n] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
__global__ void colsum_final_kernel(const float* part, float* out, int d) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= d) return;
  float s = 0.f;
  for (int c = 0; c < CS_CHUNKS; ++c) s += part[(int64_t)c * d + n];
  out[n] = s;
}
int colsum(const float* in, float* out, const ColPart& part, int M, int d, hipStream_t st) {
  if (d > part.width) VOG_FAIL(-3, "colsum: %d columns through partials laid out for %d", d, part.width);
  ::vog::launch(colsum_partial_kernel, dim3(ceil_div(d, 64), CS_CHUNKS), dim3(256), 0, st, in, part.p, M, d);
  ::vog::launch(colsum_final_kernel, dim3(ceil_div(d, 256)), dim3(256), 0, st, (const float*)part.p, out, d);
  VOG_LAUNCH_CHECK();
  return 0;
}

// y = dy where pre > 0 else 0
__global__ void relu_bwd_kernel(const float* dy, const float* act, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = act[i] > 0.f ? dy[i] : 0.f;
}

// score head: dlog[m] gathered from d mdl_outs [n_vid, nsrl, nfrm*nppf] (row m = (s = (v, f), j = arg*nppf + p),
// the inverse regroup of code/mdl_vog.py:724-737), dh[m, :] = dlog * w2 (h > 0), hw[m, :] = dlog * h (summand of d w2)
struct ScoreBwd { const float* d_outs; const float* h; const float* w2; float* dh; float* hw; float* dlog; int M, nfrm, nppf, nsrl, dh_dim; };
__global__ __launch_bounds__(256) void score_bwd_kernel(ScoreBwd a) {
  const int row = blockIdx.x, N = a.nsrl * a.nppf;
  const int s = row / N, j = row % N, v = s / a.nfrm, f = s % a.nfrm, arg = j / a.nppf, pp = j % a.nppf;
  const float dl = a.d_outs[((int64_t)v * a.nsrl + arg) * ((int64_t)a.nfrm * a.nppf) + (int64_t)f * a.nppf + pp];
  if (threadIdx.x == 0) a.dlog[row] = dl;
  for (int i = threadIdx.x; i < a.dh_dim; i += blockDim.x) {
    const float hv = a.h[(int64_t)row * a.dh_dim + i];
    a.dh[(int64_t)row * a.dh_dim + i] = hv > 0.f ? dl * a.w2[i] : 0.f;
    a.hw[(int64_t)row * a.dh_dim + i] = dl * hv;
  }
}

// ---- attention (fp32) ---------------------------------------------------------------------------------
// normalised boxes (compute_pe code/mdl_vog.py:456-463): bx[r] = (x1/w, y1/h, x2/w, y2/h, frame/nfrm_div), 8 floats per row
__global__ void norm_boxes_kernel(const float* props, int stride, float vw, float vh, float fdiv, float* bx, int rows) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* q = props + (int64_t)r * stride;
  float* o = bx + (int64_t)r * 8;
  o[0] = q[0] / vw; o[1] = q[1] / vh; o[2] = q[2] / vw; o[3] = q[3] / vh; o[4] = q[4] / fdiv; o[5] = o[6] = o[7] = 0.f;
}

void norm_boxes(const float* props, int stride, float vw, float vh, float fdiv, float* bx, int rows, hipStream_t st) {
  ::vog::launch(norm_boxes_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, st, props, stride, vw, vh, fdiv, bx, rows);
}

struct AttnRow {
  float* P;             // [S, N, N] logits in, probabilities out (softmax) | probabilities (ds)
  float* D;             // [S, N, N] dP in, d logits (before the 1/scale of Q K^T + bias) out (ds)
  const float* bx;      // [S*n, 8] or null (no relative-position bias)
  const float* w; const float* b;  // this head's Linear(5, H) row and bias entry (code/mdl_vog.py:446-451), device
  float* part;          // [S*N, 8] per-row sums of d bias . (box difference, 1) (ds)
  int S, N, n; float inv_scale;
  Drop dr; int h, H;    // dropout on the probabilities: element ((s*H + h)*N + i)*N + j of the layer's site
};

__device__ __forceinline__ float box_z(const AttnRow& a, const float* bi, const float* bj) {
  return a.w[0] * (bi[0] - bj[0]) + a.w[1] * (bi[1] - bj[1]) + a.w[2] * (bi[2] - bj[2]) + a.w[3] * (bi[3] - bj[3]) +
         a.w[4] * (bi[4] - bj[4]) + a.b[0];
}

// P[row] = softmax((P[row] + relu(w . (box_i - box_j) + b)) / scale): one wave per row (transformer_code.py:136-162)
__global__ __launch_bounds__(256) void attn_softmax_kernel(AttnRow a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.S * a.N) return;
  const int s = row / a.N, i = row % a.N;
  float* pr = a.P + (int64_t)row * a.N;
  const float* bi = a.bx ? a.bx + ((int64_t)s * a.n + i % a.n) * 8 : nullptr;
  float mx = -3.0e38f;
  for (int j = lane; j < a.N; j += 64) {
    float v = pr[j];
    if (bi) v += fmaxf(box_z(a, bi, a.bx + ((int64_t)s * a.n + j % a.n) * 8), 0.f);
    v *= a.inv_scale;
    pr[j] = v;
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
  for (int j = lane; j < a.N; j += 64) { const float e = expf(pr[j] - mx); pr[j] = e; sum += e; }
  sum = wsum(sum);
  const float inv = 1.0f / sum;
  float* dr_ = a.D + (int64_t)row * a.N;
  const unsigned long long base = (((unsigned long long)s * a.H + a.h) * a.N + i) * a.N;
  for (int j = lane; j < a.N; j += 64) {
    const float pv = pr[j] * inv;
    pr[j] = pv;
    if (a.dr.thr) dr_[j] = pv * drop_scale(a.dr, base + j);            // D := dropout(P), the operand of P V and of dV
  }
}

// D[row] = P (dP - sum_j P dP) / scale  (= d (Q K^T) = d bias); part[row] = sum_j [z > 0] D (box_i - box_j, 1)
__global__ __launch_bounds__(256) void attn_ds_kernel(AttnRow a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.S * a.N) return;
  const int s = row / a.N, i = row % a.N;
  const float* pr = a.P + (int64_t)row * a.N;
  float* dr = a.D + (int64_t)row * a.N;
  float rs = 0.f;
  const unsigned long long base = (((unsigned long long)s * a.H + a.h) * a.N + i) * a.N;
  if (a.dr.thr) for (int j = lane; j < a.N; j += 64) dr[j] *= drop_scale(a.dr, base + j);   // d P = d dropout(P) * mask (own elements)
  for (int j = lane; j < a.N; j += 64) rs += pr[j] * dr[j];
  rs = wsum(rs);
  const float* bi = a.bx ? a.bx + ((int64_t)s * a.n + i % a.n) * 8 : nullptr;
  float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = lane; j < a.N; j += 64) {
    const float ds = pr[j] * (dr[j] - rs) * a.inv_scale;
    dr[j] = ds;
    if (bi) {
      const float* bj = a.bx + ((int64_t)s * a.n + j % a.n) * 8;
      if (box_z(a, bi, bj) > 0.f) {
#pragma unroll
        for (int c = 0; c < 5; ++c) g[c] += ds * (bi[c] - bj[c]);
        g[5] += ds;
      }
    }
  }
  if (a.part) {
#pragma unroll
    for (int c = 0; c < 6; ++c) g[c] = wsum(g[c]);
    if (lane < 8) a.part[(int64_t)row * 8 + lane] = lane == 0 ? g[0] : lane == 1 ? g[1] : lane == 2 ? g[2] : lane == 3 ? g[3]
                                                    : lane == 4 ? g[4] : lane == 5 ? g[5] : 0.f;
  }
}

__global__ void pe_grad_store_kernel(const float* sum8, float* g_w, float* g_b, int h) {
  if (threadIdx.x < 5) g_w[h * 5 + threadIdx.x] = sum8[threadIdx.x];
  if (threadIdx.x == 5) g_b[h] = sum8[5];
}

// ---- seam between mul_tx's input and (obj_tx output, argument vectors): the backward of concate_vis_lang_feats +
// the (frame, argument) regroup (code/mdl_vog.py:316-344, 681-744). d_x rows ((bv, f), (arg, p)) x [dobj | dlang].
//   d_ps[(bv, f*nppf + p), c]  = sum_arg d_x[.., c]                         (every argument saw the same visual row)
//   d_lang[(b, v | 0, arg), c] = mask * sum_{(v,) f, p} d_x[.., dobj + c]   (every proposal saw the same argument vector)
struct ConcBwd { const float* dx; float* d_ps; float* d_lang; const int64_t* mask; int n_q, nc_v, nfrm, nppf, nsrl, dobj, dlang, lang_per_vid; };
__global__ void conc_bwd_ps_kernel(ConcBwd a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)a.n_q * a.nc_v * a.nfrm * a.nppf * a.dobj;
  if (i >= total) return;
  const int c = (int)(i % a.dobj);
  const int64_t r = i / a.dobj;                              // (bv, f, p)
  const int pp = (int)(r % a.nppf);
  const int64_t sf = r / a.nppf;                             // sequence (bv, f)
  const int vld = a.dobj + a.dlang;
  float s = 0.f;
  for (int ar = 0; ar < a.nsrl; ++ar) s += a.dx[((sf * a.nsrl + ar) * a.nppf + pp) * vld + c];
  a.d_ps[i] = s;
}
__global__ void conc_bwd_lang_kernel(ConcBwd a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nvl = a.lang_per_vid ? a.nc_v : 1;
  const int64_t total = (int64_t)a.n_q * nvl * a.nsrl * a.dlang;
  if (i >= total) return;
  const int c = (int)(i % a.dlang);
  const int64_t r = i / a.dlang;
  const int ar = (int)(r % a.nsrl);
  const int64_t bv = r / a.nsrl;                             // (b, v) or b
  const int vld = a.dobj + a.dlang;
  float s = 0.f;
  const int v0 = a.lang_per_vid ? 0 : 0, v1 = a.lang_per_vid ? 1 : a.nc_v;
  for (int v = v0; v < v1; ++v) {
    const int64_t q = a.lang_per_vid ? bv : bv * a.nc_v + v;
    for (int f = 0; f < a.nfrm; ++f)
      for (int pp = 0; pp < a.nppf; ++pp)
        s += a.dx[(((q * a.nfrm + f) * a.nsrl + ar) * a.nppf + pp) * vld + a.dobj + c];
  }
  a.d_lang[i] = a.mask && a.mask[r] == 0 ? 0.f : s;
}

// ---- Linear (+ ReLU): y = act(x W^T + b), rows optionally replicated downstream (segment rows: concat_prop_seg_feats)
// dpre[m, n] = [y > 0] * sum_{j < rep} dy[(m*rep + j) * ldy + n]
__global__ void lin_dpre_kernel(const float* dy, int64_t ldy, int rep, const float* y, int relu, float* dpre, int M, int N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int n = (int)(i % N);
  const int64_t m = i / N;
  float s = 0.f;
  for (int j = 0; j < rep; ++j) s += dy[(m * rep + j) * ldy + n];
  dpre[i] = (!relu || y[i] > 0.f) ? s : 0.f;
}
void lin_dpre(const float* dy, int64_t ldy, int rep, const float* y, int relu, float* dpre, int M, int N, hipStream_t st) {
  ::vog::launch(lin_dpre_kernel, dim3((unsigned)(((int64_t)M * N + 255) / 256)), dim3(256), 0, st, dy, ldy, rep, y, relu, dpre, M, N);
}

__global__ void add_kernel(const float* a, const float* b, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

}  // namespace vog

using namespace vog;

struct TailBufs {
  float *t, *x1, *u, *y, *dy, *du, *dx1, *dt, *tmp, *pre1, *dpre1, *df, *h, *dh, *hw; float2 *st1, *st2; float* dlog; ColPart part;
  int64_t bytes;
};
static TailBufs tail_layout(void* base, int M, int d, int H1, int HD) {    // (HD = 0: a tail without the score head)
  Carve c(base, 1, false);
  TailBufs b;
  for (float** p : {&b.t, &b.x1, &b.u, &b.y, &b.dy, &b.du, &b.dx1, &b.dt, &b.tmp}) *p = c.take<float>((int64_t)M * d);
  for (float** p : {&b.pre1, &b.dpre1, &b.df}) *p = c.take<float>((int64_t)M * H1);
  for (float** p : {&b.h, &b.dh, &b.hw}) *p = c.take<float>((int64_t)M * HD);
  b.st1 = c.take<float2>(M); b.st2 = c.take<float2>(M);
  b.dlog = c.take<float>((M + 3) / 4 * 4);
  b.part = c.colpart(std::max({d, H1, HD}));           // the matrices summed by columns: d (LayerNorm, b2), dh (b1), dhead wide
  b.bytes = c.bytes();
  return b;
}
extern "C" int64_t vog_mul_tail_bwd_scratch_bytes(int M, int d, int dh, int dhead) {
  if (M <= 0 || d <= 0 || dh <= 0 || dhead < 0) return -1;
  return tail_layout(nullptr, M, d, dh, dhead).bytes;
}

extern "C" int vog_mul_tail_bwd(const vog_tail_bwd_args* a, void* stream) {
  VOG_CHECK_ARG(a && a->attn && a->x && a->scratch && a->M > 0 && a->d > 0 && a->dh > 0);
  VOG_CHECK_ARG(a->wo && a->ln1g && a->ln1b && a->w1 && a->b1 && a->w2 && a->b2 && a->ln2g && a->ln2b);
  // no_head: a layer that is not followed by the score head - its output gradient d_y comes from the caller; without
  // d_y only the forward is recomputed (y_out = the layer's output)
  const bool head = !a->no_head;
  const bool fwd_only = a->no_head && !a->d_y;
  if (fwd_only) VOG_CHECK_ARG(a->y_out);
  if (head) {
    VOG_CHECK_ARG(a->d_mdl_outs && a->dhead > 0 && a->wl && a->bl && a->wl2);
    VOG_CHECK_ARG(a->M == a->n_vid * a->nfrm * a->nsrl * a->nppf);
  }
  if ((int64_t)a->scratch_bytes < vog_mul_tail_bwd_scratch_bytes(a->M, a->d, a->dh, head ? a->dhead : 0))
    VOG_FAIL(-2, "vog_mul_tail_bwd: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const int M = a->M, d = a->d, H1 = a->dh, HD = head ? a->dhead : 0;
  const TailBufs b = tail_layout(a->scratch, M, d, H1, HD);
  float *t = b.t, *x1 = b.x1, *u = b.u, *y = b.y, *dy = b.dy, *du = b.du, *dx1 = b.dx1, *dt = b.dt, *tmp = b.tmp;
  float *pre1 = b.pre1, *dpre1 = b.dpre1, *df = b.df, *h = b.h, *dh = b.dh, *hw = b.hw, *dlog = b.dlog;
  float2 *st1 = b.st1, *st2 = b.st2;
  const ColPart part = b.part;
  const int64_t nd = (int64_t)M * d, n1 = (int64_t)M * H1;
  auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  // ---- recompute the forward in fp32
  VOG_TRY(gemm_f32(a->attn, d, 1, a->wo, 1, d, t, d, nullptr, 0, M, d, d, st));                    // a Wo^T   (Wo [d_out, d_in])
  const Drop dr1 = make_drop(a->drop_p, a->drop_seed, a->drop_site + 1), dr2 = make_drop(a->drop_p, a->drop_seed, a->drop_site + 2);
  ::vog::launch(ln_fwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, t, a->x, a->ln1g, a->ln1b, x1, st1, M, d, dr1);   // t = drop(t) + x
  VOG_TRY(gemm_f32(x1, d, 1, a->w1, 1, d, pre1, H1, a->b1, 0, M, H1, d, st));                       // pre1 (relu applied on use)
  ::vog::launch(relu_bwd_kernel, blocks(n1), dim3(256), 0, st, pre1, pre1, df, n1);                  // df = relu(pre1) (reused as f)
  VOG_TRY(gemm_f32(df, H1, 1, a->w2, 1, H1, u, d, a->b2, 0, M, d, H1, st));                          // f W2^T + b2
  ::vog::launch(ln_fwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, u, (const float*)x1, a->ln2g, a->ln2b, y, st2, M, d, dr2);   // u = drop(u) + x1
  if (a->y_out) VOG_TRY(dev_copy(a->y_out, y, (size_t)nd * 4, st));   // the layer's output
  if (fwd_only) { VOG_LAUNCH_CHECK(); return 0; }
  const float* dyp = a->d_y;
  if (head) {
    VOG_TRY(gemm_f32(y, d, 1, a->wl, 1, d, h, HD, a->bl, 1, M, HD, d, st));                          // h = relu(y Wl^T + bl)
    // ---- score head
    ScoreBwd sb{a->d_mdl_outs, h, a->wl2, dh, hw, dlog, M, a->nfrm, a->nppf, a->nsrl, HD};
    ::vog::launch(score_bwd_kernel, dim3(M), dim3(256), 0, st, sb);
    if (a->g_wl2) VOG_TRY(colsum(hw, a->g_wl2, part, M, HD, st));   // d lin2.2.weight
    if (a->g_bl2) VOG_TRY(colsum(dlog, a->g_bl2, part, M, 1, st));                 // d lin2.2.bias
    if (a->g_wl) VOG_TRY(gemm_f32(dh, 1, HD, y, d, 1, a->g_wl, d, nullptr, 0, HD, d, M, st));        // d lin2.0.weight = dh^T y
    if (a->g_bl) VOG_TRY(colsum(dh, a->g_bl, part, M, HD, st));
    VOG_TRY(gemm_f32(dh, HD, 1, a->wl, d, 1, dy, d, nullptr, 0, M, d, HD, st));                      // dy = dh Wl
    dyp = dy;
  }
  // ---- LayerNorm 2
  ::vog::launch(ln_bwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, dyp, (const float*)nullptr, (const float*)u,
                (const float2*)st2, a->ln2g, du, tmp, (float*)nullptr, M, d);
  if (a->g_ln2g) VOG_TRY(colsum(tmp, a->g_ln2g, part, M, d, st));
  if (a->g_ln2b) VOG_TRY(colsum(dyp, a->g_ln2b, part, M, d, st));
  // ---- FFN (dum = the gradient behind the feed-forward sub-layer's dropout; du itself is the residual path)
  const float* dum = du;
  if (dr2.thr) { mask_mul(du, dy, dr2, nd, st); dum = dy; }
  if (a->g_w2) VOG_TRY(gemm_f32(dum, 1, d, df, H1, 1, a->g_w2, H1, nullptr, 0, d, H1, M, st));       // d W2 = du^T f
  if (a->g_b2) VOG_TRY(colsum(dum, a->g_b2, part, M, d, st));
  VOG_TRY(gemm_f32(dum, d, 1, a->w2, H1, 1, dpre1, H1, nullptr, 0, M, H1, d, st));                   // df = du W2
  ::vog::launch(relu_bwd_kernel, blocks(n1), dim3(256), 0, st, (const float*)dpre1, (const float*)pre1, dpre1, n1);
  if (a->g_w1) VOG_TRY(gemm_f32(dpre1, 1, H1, x1, d, 1, a->g_w1, d, nullptr, 0, H1, d, M, st));      // d W1 = dpre1^T x1
  if (a->g_b1) VOG_TRY(colsum(dpre1, a->g_b1, part, M, H1, st));
  VOG_TRY(gemm_f32(dpre1, H1, 1, a->w1, d, 1, dx1, d, nullptr, 0, M, d, H1, st));                    // dpre1 W1
  // ---- LayerNorm 1 (dx1 = du + dpre1 W1)
  ::vog::launch(ln_bwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, (const float*)dx1, (const float*)du, (const float*)t,
                (const float2*)st1, a->ln1g, dt, tmp, dy, M, d);                                       // dy := dx1 + du (summand of d beta)
  if (a->g_ln1g) VOG_TRY(colsum(tmp, a->g_ln1g, part, M, d, st));
  if (a->g_ln1b) VOG_TRY(colsum(dy, a->g_ln1b, part, M, d, st));
  // ---- Wo and the two inputs (dtm = the gradient behind the attention sub-layer's dropout)
  const float* dtm = dt;
  if (dr1.thr) { mask_mul(dt, tmp, dr1, nd, st); dtm = tmp; }
  if (a->g_wo) VOG_TRY(gemm_f32(dtm, 1, d, a->attn, d, 1, a->g_wo, d, nullptr, 0, d, d, M, st));     // d Wo = dt^T a
  if (a->d_attn) VOG_TRY(gemm_f32(dtm, d, 1, a->wo, d, 1, a->d_attn, d, nullptr, 0, M, d, d, st));   // da = dt Wo
  if (a->d_x) VOG_TRY(dev_copy(a->d_x, dt, (size_t)nd * 4, st));      // dx = dt
  VOG_LAUNCH_CHECK();
  return 0;
}

// ---- attention + Q/K/V projections of one (Rel)EncoderLayer in fp32: forward (concatenated heads) and backward ----
struct AttnBufs { float *q, *k, *v, *dq, *dk, *dv, *P, *D, *bx, *part; ColPart cpart; float* sum8; int64_t bytes; };
static AttnBufs attn_layout(void* base, int S, int N, int n, int d) {
  Carve c(base, 4, true);
  AttnBufs b;
  const int64_t M = (int64_t)S * N;
  for (float** p : {&b.q, &b.k, &b.v, &b.dq, &b.dk, &b.dv}) *p = c.take<float>(M * d);
  b.P = c.take<float>(M * N); b.D = c.take<float>(M * N);            // [S, N, N]: one head's probabilities / their gradient
  b.bx = c.take<float>((int64_t)S * n * 8);                            // normalised boxes
  b.part = c.take<float>(M * 8);                                       // per-row sums of d bias, summed by columns into sum8
  b.cpart = c.colpart(8); b.sum8 = c.take<float>(8);
  b.bytes = c.bytes();
  return b;
}
extern "C" int64_t vog_attn_f32_scratch_bytes(int S, int N, int n, int d) {
  if (S <= 0 || N <= 0 || n <= 0 || d <= 0) return -1;
  return attn_layout(nullptr, S, N, n, d).bytes;
}

// vl (vog_attn_f32_vl): the input as its factors - q, k, v come from vl_forward, the gradients behind dq, dk, dv from vl_backward
static int attn_f32_body(const vog_attn_f32_args* a, const vog_attn_vl* vl, void* stream) {
  VOG_CHECK_ARG(a && (vl || a->x) && a->wq && a->wk && a->wv && a->scratch && a->S > 0 && a->N > 0 && a->n > 0 && a->d > 0 && a->n_heads > 0);
  VOG_CHECK_ARG((a->N % a->n) == 0 && a->n_heads <= a->d);
  if (vl) VOG_TRY(vl_check(vl, a->d_x, a->S, a->N, a->n, a->d));
  const bool bwd = a->d_cat != nullptr, rel = a->props != nullptr;
  if (rel) VOG_CHECK_ARG(a->pe_w && a->pe_b && a->prop_stride >= 5 && a->vid_w > 0.f && a->vid_h > 0.f && a->nfrm_div > 0.f);
  // backward: every g_* and d_x may be NULL (a frozen weight / an input nothing below needs): its GEMMs are skipped
  if (bwd && rel) VOG_CHECK_ARG(!a->g_pe_w == !a->g_pe_b);
  const bool any_dx = a->d_x || (vl && (vl->d_ps || vl->d_lang));
  const bool need_dq = a->g_wq || any_dx, need_dk = a->g_wk || any_dx, need_dv = a->g_wv || any_dx;
  const bool pe_grad = bwd && rel && a->g_pe_w;
  if (!bwd) VOG_CHECK_ARG(a->cat_out);
  if ((int64_t)a->scratch_bytes < vog_attn_f32_scratch_bytes(a->S, a->N, a->n, a->d)) VOG_FAIL(-2, "vog_attn_f32: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const int S = a->S, N = a->N, n = a->n, d = a->d, H = a->n_heads, M = S * N;
  const AttnBufs b = attn_layout(a->scratch, S, N, n, d);
  float *q = b.q, *k = b.k, *v = b.v, *dq = b.dq, *dk = b.dk, *dv = b.dv, *P = b.P, *D = b.D, *bx = b.bx, *part = b.part, *sum8 = b.sum8;
  const int64_t nn = (int64_t)N * N;
  // q, k, v = x W^T  (transformer_code.py:136-150; no bias)
  if (vl) {
    VOG_TRY(vl_forward(vl, a->wq, a->wk, a->wv, q, k, v, n, st));
  } else {
    VOG_TRY(gemm_f32(a->x, d, 1, a->wq, 1, d, q, d, nullptr, 0, M, d, d, st));
    VOG_TRY(gemm_f32(a->x, d, 1, a->wk, 1, d, k, d, nullptr, 0, M, d, d, st));
    VOG_TRY(gemm_f32(a->x, d, 1, a->wv, 1, d, v, d, nullptr, 0, M, d, d, st));
  }
  if (rel)
    ::vog::launch(norm_boxes_kernel, dim3(ceil_div(S * n, 256)), dim3(256), 0, st, a->props, a->prop_stride, a->vid_w, a->vid_h,
                  a->nfrm_div, bx, S * n);
  const Drop drp = make_drop(a->drop_p, a->drop_seed, a->drop_site);
  const int chunk = (d + H - 1) / H;                       // torch.chunk split sizes (transformer_code.py:66-67)
  const float inv_scale = 1.0f / sqrtf((float)d);          // scale = sqrt(d_model)
  const int64_t sx = (int64_t)N * d;
  for (int h = 0; h < H; ++h) {
    const int off = h * chunk, dh = (d - off) < chunk ? (d - off) : chunk;
    if (dh <= 0) VOG_FAIL(-1, "vog_attn_f32: %d heads do not split %d features", H, d);
    // logits = Q_h K_h^T, then the softmax with the box bias
    VOG_TRY(gemm_f32_b(q + off, d, 1, sx, k + off, 1, d, sx, P, N, nn, nullptr, 0, 0, N, N, dh, S, st));
    AttnRow ar{P, D, rel ? bx : nullptr, rel ? a->pe_w + h * 5 : nullptr, rel ? a->pe_b + h : nullptr, pe_grad ? part : nullptr,
               S, N, n, inv_scale, drp, h, H};
    ::vog::launch(attn_softmax_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, ar);
    const float* Pd = drp.thr ? D : P;                                   // dropout(P) (D holds it until dP overwrites it)
    if (a->cat_out)
      VOG_TRY(gemm_f32_b(Pd, N, 1, nn, v + off, d, 1, sx, a->cat_out + off, d, sx, nullptr, 0, 0, N, dh, N, S, st));  // O_h = drop(P) V_h
    if (!bwd) continue;
    if (need_dv)
      VOG_TRY(gemm_f32_b(Pd, 1, N, nn, a->d_cat + off, d, 1, sx, dv + off, d, sx, nullptr, 0, 0, N, dh, N, S, st));   // dV_h = drop(P)^T dO_h
    if (!need_dq && !need_dk && !pe_grad) continue;
    VOG_TRY(gemm_f32_b(a->d_cat + off, d, 1, sx, v + off, 1, d, sx, D, N, nn, nullptr, 0, 0, N, N, dh, S, st));       // d drop(P) = dO_h V_h^T
    ::vog::launch(attn_ds_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, ar);
    if (need_dq) VOG_TRY(gemm_f32_b(D, N, 1, nn, k + off, d, 1, sx, dq + off, d, sx, nullptr, 0, 0, N, dh, N, S, st));   // dQ_h = dS K_h
    if (need_dk) VOG_TRY(gemm_f32_b(D, 1, N, nn, q + off, d, 1, sx, dk + off, d, sx, nullptr, 0, 0, N, dh, N, S, st));   // dK_h = dS^T Q_h
    if (pe_grad) {
      VOG_TRY(colsum(part, sum8, b.cpart, M, 8, st));
      ::vog::launch(pe_grad_store_kernel, dim3(1), dim3(64), 0, st, (const float*)sum8, a->g_pe_w, a->g_pe_b, h);
    }
  }
  if (bwd && vl) {
    VOG_TRY(vl_backward(vl, a->wq, a->wk, a->wv, dq, dk, dv, a->g_wq, a->g_wk, a->g_wv, n, st));
  } else if (bwd) {
    if (a->g_wq) VOG_TRY(gemm_f32(dq, 1, d, a->x, d, 1, a->g_wq, d, nullptr, 0, d, d, M, st));      // d Wq = dQ^T x
    if (a->g_wk) VOG_TRY(gemm_f32(dk, 1, d, a->x, d, 1, a->g_wk, d, nullptr, 0, d, d, M, st));
    if (a->g_wv) VOG_TRY(gemm_f32(dv, 1, d, a->x, d, 1, a->g_wv, d, nullptr, 0, d, d, M, st));
    if (a->d_x) {
      VOG_TRY(gemm_f32(dq, d, 1, a->wq, d, 1, a->d_x, d, nullptr, 0, M, d, d, st, a->accumulate_dx ? 1 : 0));   // dx (+)= dQ Wq + dK Wk + dV Wv
      VOG_TRY(gemm_f32(dk, d, 1, a->wk, d, 1, a->d_x, d, nullptr, 0, M, d, d, st, 1));
      VOG_TRY(gemm_f32(dv, d, 1, a->wv, d, 1, a->d_x, d, nullptr, 0, M, d, d, st, 1));
    }
  }
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_attn_f32(const vog_attn_f32_args* a, void* stream) { return attn_f32_body(a, nullptr, stream); }

extern "C" int vog_conc_f32_bwd(const float* d_x, float* d_ps, float* d_lang, const int64_t* inds_msk, int n_q, int nc_v, int nfrm,
                                int nppf, int nsrl, int dobj, int dlang, int lang_per_vid, void* stream) {
  VOG_CHECK_ARG(d_x && d_ps && n_q > 0 && nc_v > 0 && nfrm > 0 && nppf > 0 && nsrl > 0 && dobj > 0 && dlang >= 0);
  ConcBwd a{d_x, d_ps, d_lang, inds_msk, n_q, nc_v, nfrm, nppf, nsrl, dobj, dlang, lang_per_vid};
  const int64_t t1 = (int64_t)n_q * nc_v * nfrm * nppf * dobj;
  ::vog::launch(conc_bwd_ps_kernel, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  if (d_lang && dlang > 0) {
    const int64_t t2 = (int64_t)n_q * (lang_per_vid ? nc_v : 1) * nsrl * dlang;
    ::vog::launch(conc_bwd_lang_kernel, dim3((unsigned)((t2 + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  }
  VOG_LAUNCH_CHECK();
  return 0;
}

// ---- the attention operators on the factors of mul_tx's layer-0 input (vog_attn_vl, include/vog_hip.h): T = Pv + Pl per token,
// and the two sums that take dT back to the factors. Memory-bound row kernels on one grid: x = sequence, y = 64-column block,
// z = which of q / k / v; V = 4 (16-byte accesses: d a multiple of 4 - every matrix here is d wide and starts on a 16-byte
// carve, so dobj does not matter) | 1. A workgroup is 64 / V column lanes x 4 V row lanes.
namespace vog {

template <int V> struct VlT { typedef float4 type; };
template <> struct VlT<1> { typedef float type; };
__device__ __forceinline__ float4 vl_add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float vl_add(float a, float b) { return a + b; }
__device__ __forceinline__ void vl_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void vl_zero(float& a) { a = 0.f; }
// one of three kernel arguments by a block-uniform index (selects, not an indexed copy of the array)
template <typename P> __device__ __forceinline__ P vl_pick(P const (&p)[3], int t) { return t == 0 ? p[0] : t == 1 ? p[1] : p[2]; }

// out_t[(s, arg, p), :] = pv_t[(s, p), :] + [mask(g, arg)] pl_t[(g, arg), :], g = s / spg
struct VlExpand { const float* pv[3]; const float* pl[3]; float* out[3]; const int64_t* mask; int n, nsrl, d, spg; };
template <int V>
__global__ __launch_bounds__(256) void vl_expand_kernel(VlExpand a) {
  typedef typename VlT<V>::type T;
  constexpr int CL = 64 / V, RL = 256 / CL;
  const int s = blockIdx.x, t = blockIdx.z, c = blockIdx.y * 64 + (threadIdx.x % CL) * V, r = threadIdx.x / CL;
  if (c >= a.d) return;
  const int N = a.nsrl * a.n;
  const int64_t g = s / a.spg;
  const float* pv = vl_pick(a.pv, t) + (int64_t)s * a.n * a.d + c;
  const float* pl = vl_pick(a.pl, t) + g * a.nsrl * a.d + c;
  float* o = vl_pick(a.out, t) + (int64_t)s * N * a.d + c;
  for (int i = r; i < N; i += RL) {
    const int arg = i / a.n, p = i - arg * a.n;
    T x = *reinterpret_cast<const T*>(pv + (int64_t)p * a.d);
    if (!a.mask || a.mask[g * a.nsrl + arg] != 0) x = vl_add(x, *reinterpret_cast<const T*>(pl + (int64_t)arg * a.d));
    *reinterpret_cast<T*>(o + (int64_t)i * a.d) = x;
  }
}

// One read of dt_t [(s, arg, p), :]: dpv_t[(s, p), :] = sum_arg dt (ascending arg) and part_t[(s, arg), :] = sum_p dt - a row
// lane adds its p = r, r + 4 V, .. in that order, then the row lanes are added in lane order through LDS. Arguments go in chunks
// of AC, whose sums live in registers; a later chunk continues the running dpv row it wrote itself.
struct VlReduce { const float* dt[3]; float* dpv[3]; float* part[3]; int n, nsrl, d; };
template <int V>
__global__ __launch_bounds__(256) void vl_reduce_kernel(VlReduce a) {
  typedef typename VlT<V>::type T;
  constexpr int CL = 64 / V, RL = 256 / CL, AC = 8;
  __shared__ __attribute__((aligned(16))) T red[AC][256];
  const int tid = threadIdx.x, cl = tid % CL, r = tid / CL;
  const int s = blockIdx.x, t = blockIdx.z, c0 = blockIdx.y * 64, c = c0 + cl * V;
  const bool on = c < a.d;
  const float* dt = vl_pick(a.dt, t) + (int64_t)s * a.nsrl * a.n * a.d + c;
  float* dpv = vl_pick(a.dpv, t) + (int64_t)s * a.n * a.d + c;
  float* part = vl_pick(a.part, t) + (int64_t)s * a.nsrl * a.d + c0;
  for (int a0 = 0; a0 < a.nsrl; a0 += AC) {
    const int na = a.nsrl - a0 < AC ? a.nsrl - a0 : AC;
    T acc[AC];
#pragma unroll
    for (int j = 0; j < AC; ++j) vl_zero(acc[j]);
    if (on)
      for (int p = r; p < a.n; p += RL) {
        T sv;
        if (a0) sv = *reinterpret_cast<const T*>(dpv + (int64_t)p * a.d); else vl_zero(sv);
#pragma unroll
        for (int j = 0; j < AC; ++j)
          if (j < na) {
            const T x = *reinterpret_cast<const T*>(dt + ((int64_t)(a0 + j) * a.n + p) * a.d);
            sv = vl_add(sv, x);
            acc[j] = vl_add(acc[j], x);
          }
        *reinterpret_cast<T*>(dpv + (int64_t)p * a.d) = sv;
      }
#pragma unroll
    for (int j = 0; j < AC; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int e = tid; e < na * CL; e += 256) {
      const int j = e / CL, l = e - j * CL;
      if (c0 + l * V < a.d) {
        T u = red[j][l];
        for (int q = 1; q < RL; ++q) u = vl_add(u, red[j][q * CL + l]);
        *reinterpret_cast<T*>(part + (int64_t)(a0 + j) * a.d + l * V) = u;
      }
    }
    __syncthreads();
  }
}

// dpl_t[(g, arg), :] = [mask(g, arg)] sum over the spg sequences of group g, ascending s, of part_t[(s, arg), :]
struct VlGroups { const float* part[3]; float* dpl[3]; const int64_t* mask; int nsrl, d, spg; int64_t rows; };
template <int V>
__global__ __launch_bounds__(256) void vl_reduce_groups_kernel(VlGroups a) {
  typedef typename VlT<V>::type T;
  const int dv = a.d / V, t = blockIdx.z;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.rows * dv) return;
  const int c = (int)(i % dv) * V;
  const int64_t row = i / dv, g = row / a.nsrl;
  const int arg = (int)(row - g * a.nsrl);
  const float* part = vl_pick(a.part, t) + c;
  T u;
  vl_zero(u);
  if (!a.mask || a.mask[row] != 0)
    for (int64_t s = g * a.spg; s < (g + 1) * a.spg; ++s) u = vl_add(u, *reinterpret_cast<const T*>(part + (s * a.nsrl + arg) * a.d));
  *reinterpret_cast<T*>(vl_pick(a.dpl, t) + row * a.d + c) = u;
}

namespace {
struct VlGeo { int S, Sn, G, L, spg, d; };                  // Sn = S*n visual rows, L = G*nsrl argument rows
bool vl_geo(int n_q, int nc_v, int nfrm, int n, int nsrl, int dobj, int dlang, int lang_per_vid, VlGeo* o) {
  if (n_q <= 0 || nc_v <= 0 || nfrm <= 0 || n <= 0 || nsrl <= 0 || dobj <= 0 || dlang <= 0) return false;
  const int64_t S = (int64_t)n_q * nc_v * nfrm, lim = (int64_t)1 << 31;
  if (S >= lim || S * n * nsrl >= lim || (int64_t)dobj + dlang >= lim) return false;   // (the operators index tokens with int)
  const int G = n_q * (lang_per_vid ? nc_v : 1);
  *o = VlGeo{(int)S, (int)(S * n), G, G * nsrl, (int)(S / G), dobj + dlang};
  return true;
}
struct VlBufs { float *pv[3], *pl[3], *dpv[3], *dpl[3], *part[3]; int64_t bytes; };
VlBufs vl_layout(void* base, const VlGeo& g, int nsrl) {
  Carve c(base, 4, true);
  VlBufs b;
  for (int t = 0; t < 3; ++t) { b.pv[t] = c.take<float>((int64_t)g.Sn * g.d); b.pl[t] = c.take<float>((int64_t)g.L * g.d); }
  for (int t = 0; t < 3; ++t) { b.dpv[t] = c.take<float>((int64_t)g.Sn * g.d); b.dpl[t] = c.take<float>((int64_t)g.L * g.d); }
  for (int t = 0; t < 3; ++t) b.part[t] = c.take<float>((int64_t)g.S * nsrl * g.d);   // per-sequence sums over the proposals
  b.bytes = c.bytes();
  return b;
}
}  // namespace

int vl_check(const vog_attn_vl* vl, const float* d_x, int S, int N, int n, int d) {
  VOG_CHECK_ARG(vl->ps && vl->lang && vl->scratch);
  VOG_CHECK_ARG(vl->dlang > 0);                                     // no language part: nothing to factor, use the dense entry
  VlGeo g;
  VOG_CHECK_ARG(vl_geo(vl->n_q, vl->nc_v, vl->nfrm, n, vl->nsrl, vl->dobj, vl->dlang, vl->lang_per_vid, &g));
  VOG_CHECK_ARG(d_x == nullptr);                                    // the input's gradient is d_ps / d_lang
  VOG_CHECK_ARG(S == g.S && N == vl->nsrl * n && d == g.d);
  if ((int64_t)vl->scratch_bytes < vl_layout(nullptr, g, vl->nsrl).bytes) VOG_FAIL(-2, "vog_attn_vl: scratch too small");
  return 0;
}

int vl_forward(const vog_attn_vl* vl, const float* wq, const float* wk, const float* wv, float* q, float* k, float* v, int n,
               hipStream_t st) {
  VlGeo g;
  VOG_CHECK_ARG(vl_geo(vl->n_q, vl->nc_v, vl->nfrm, n, vl->nsrl, vl->dobj, vl->dlang, vl->lang_per_vid, &g));
  const VlBufs b = vl_layout(vl->scratch, g, vl->nsrl);
  const int d = g.d, dobj = vl->dobj, dlang = vl->dlang;
  const float* w[3] = {wq, wk, wv};
  for (int t = 0; t < 3; ++t) {                                     // Pv_t = ps W_t[:, :dobj]^T, Pl_t = lang W_t[:, dobj:]^T
    VOG_TRY(gemm_f32(vl->ps, dobj, 1, w[t], 1, d, b.pv[t], d, nullptr, 0, g.Sn, d, dobj, st));
    VOG_TRY(gemm_f32(vl->lang, dlang, 1, w[t] + dobj, 1, d, b.pl[t], d, nullptr, 0, g.L, d, dlang, st));
  }
  const VlExpand e{{b.pv[0], b.pv[1], b.pv[2]}, {b.pl[0], b.pl[1], b.pl[2]}, {q, k, v}, vl->inds_msk, n, vl->nsrl, d, g.spg};
  const dim3 grid(g.S, ceil_div(d, 64), 3);
  if (d % 4 == 0) ::vog::launch(vl_expand_kernel<4>, grid, dim3(256), 0, st, e);
  else ::vog::launch(vl_expand_kernel<1>, grid, dim3(256), 0, st, e);
  ++train_int(TRAIN_ATTN_VL_LAUNCHES);
  VOG_LAUNCH_CHECK();
  return 0;
}

int vl_backward(const vog_attn_vl* vl, const float* wq, const float* wk, const float* wv, const float* dq, const float* dk,
                const float* dv, float* g_wq, float* g_wk, float* g_wv, int n, hipStream_t st) {
  VlGeo g;
  VOG_CHECK_ARG(vl_geo(vl->n_q, vl->nc_v, vl->nfrm, n, vl->nsrl, vl->dobj, vl->dlang, vl->lang_per_vid, &g));
  const VlBufs b = vl_layout(vl->scratch, g, vl->nsrl);
  const int d = g.d, dobj = vl->dobj, dlang = vl->dlang;
  const float* w[3] = {wq, wk, wv};
  const float* dt[3] = {dq, dk, dv};
  float* gw[3] = {g_wq, g_wk, g_wv};
  const bool din = vl->d_ps || vl->d_lang;
  int use[3], nu = 0;                                               // the ones of q / k / v whose gradient something needs
  for (int t = 0; t < 3; ++t)
    if (gw[t] || din) use[nu++] = t;
  if (nu == 0) return 0;
  VlReduce r{};
  VlGroups gr{};
  for (int i = 0; i < 3; ++i) {                                     // (slots behind nu repeat the last one: never launched)
    const int t = use[i < nu ? i : nu - 1];
    r.dt[i] = dt[t]; r.dpv[i] = b.dpv[t]; r.part[i] = b.part[t];
    gr.part[i] = b.part[t]; gr.dpl[i] = b.dpl[t];
  }
  r.n = n; r.nsrl = vl->nsrl; r.d = d;
  gr.mask = vl->inds_msk; gr.nsrl = vl->nsrl; gr.d = d; gr.spg = g.spg; gr.rows = g.L;
  const dim3 grid(g.S, ceil_div(d, 64), nu);
  const bool vec = d % 4 == 0;
  if (vec) ::vog::launch(vl_reduce_kernel<4>, grid, dim3(256), 0, st, r);
  else ::vog::launch(vl_reduce_kernel<1>, grid, dim3(256), 0, st, r);
  ++train_int(TRAIN_ATTN_VL_LAUNCHES);
  if (g_wq || g_wk || g_wv || vl->d_lang) {                         // (d_ps alone needs no dPl)
    const int64_t el = (int64_t)g.L * (d / (vec ? 4 : 1));
    const dim3 gg((unsigned)((el + 255) / 256), 1, nu);
    if (vec) ::vog::launch(vl_reduce_groups_kernel<4>, gg, dim3(256), 0, st, gr);
    else ::vog::launch(vl_reduce_groups_kernel<1>, gg, dim3(256), 0, st, gr);
    ++train_int(TRAIN_ATTN_VL_LAUNCHES);
  }
  for (int i = 0; i < nu; ++i) {                                    // g_w_t = [dPv_t^T ps | dPl_t^T lang] (dPl is zero where the mask is)
    const int t = use[i];
    if (!gw[t]) continue;
    VOG_TRY(gemm_f32(b.dpv[t], 1, d, vl->ps, dobj, 1, gw[t], d, nullptr, 0, d, dobj, g.Sn, st));
    VOG_TRY(gemm_f32(b.dpl[t], 1, d, vl->lang, dlang, 1, gw[t] + dobj, d, nullptr, 0, d, dlang, g.L, st));
  }
  if (vl->d_ps)                                                     // d_ps (+)= sum_t dPv_t W_t[:, :dobj]
    for (int i = 0; i < nu; ++i)
      VOG_TRY(gemm_f32(b.dpv[use[i]], d, 1, w[use[i]], d, 1, vl->d_ps, dobj, nullptr, 0, g.Sn, dobj, d, st, (i || vl->accumulate) ? 1 : 0));
  if (vl->d_lang)                                                   // d_lang (+)= sum_t dPl_t W_t[:, dobj:]
    for (int i = 0; i < nu; ++i)
      VOG_TRY(gemm_f32(b.dpl[use[i]], d, 1, w[use[i]] + dobj, d, 1, vl->d_lang, dlang, nullptr, 0, g.L, dlang, d, st, (i || vl->accumulate) ? 1 : 0));
  VOG_LAUNCH_CHECK();
  return 0;
}

}  // namespace vog

extern "C" int64_t vog_attn_vl_scratch_bytes(int n_q, int nc_v, int nfrm, int n, int nsrl, int dobj, int dlang, int lang_per_vid) {
  VlGeo g;
  if (!vl_geo(n_q, nc_v, nfrm, n, nsrl, dobj, dlang, lang_per_vid, &g)) return -1;
  return vl_layout(nullptr, g, nsrl).bytes;
}

extern "C" int vog_attn_f32_vl(const vog_attn_f32_args* a, const vog_attn_vl* vl, void* stream) {
  VOG_CHECK_ARG(vl);
  return attn_f32_body(a, vl, stream);
}

struct LinearBufs { float *y, *dpre; ColPart part; int64_t bytes; };   // y, dpre [M, N]
static LinearBufs linear_layout(void* base, int M, int N) {
  Carve c(base, 1, false);
  LinearBufs b;
  b.y = c.take<float>((int64_t)M * N); b.dpre = c.take<float>((int64_t)M * N);
  b.part = c.colpart(N);
  b.bytes = c.bytes();
  return b;
}
extern "C" int64_t vog_linear_f32_scratch_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return -1;
  return linear_layout(nullptr, M, N).bytes;
}

extern "C" int vog_linear_f32(const vog_linear_f32_args* a, void* stream) {
  VOG_CHECK_ARG(a && a->x && a->w && a->M > 0 && a->N > 0 && a->K > 0 && a->scratch);
  if ((int64_t)a->scratch_bytes < vog_linear_f32_scratch_bytes(a->M, a->N)) VOG_FAIL(-2, "vog_linear_f32: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const int M = a->M, N = a->N, K = a->K;
  const LinearBufs b = linear_layout(a->scratch, M, N);
  float *y = a->y ? a->y : b.y, *dpre = b.dpre;
  const int64_t ldx = a->ldx > 0 ? a->ldx : K;
  VOG_TRY(gemm_f32(a->x, ldx, 1, a->w, 1, K, y, N, a->b, a->relu, M, N, K, st));                     // y = act(x W^T + b)
  if (!a->dy) { VOG_LAUNCH_CHECK(); return 0; }
  VOG_CHECK_ARG(a->rep >= 1);                                          // (g_w / g_b / d_x: each optional, NULL = skipped)
  const int64_t ldy = a->ldy > 0 ? a->ldy : N;
  lin_dpre(a->dy, ldy, a->rep, y, a->relu, dpre, M, N, st);
  if (a->g_w) VOG_TRY(gemm_f32(dpre, 1, N, a->x, ldx, 1, a->g_w, K, nullptr, 0, N, K, M, st));      // d W = dpre^T x
  if (a->g_b) VOG_TRY(colsum(dpre, a->g_b, b.part, M, N, st));
  if (a->d_x) VOG_TRY(gemm_f32(dpre, N, 1, a->w, K, 1, a->d_x, a->ldx > 0 ? a->ldx : K, nullptr, 0, M, K, N, st, a->accumulate_dx ? 1 : 0));
  VOG_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================================
// The remaining forward pieces of the fp32 training path (concatenations, score head) and the optimizer step
// =====================================================================================================================
namespace vog {

// out[m, :Na] = a[m / rep_a], out[m, Na:] = b[m / rep_b]        (concat_prop_seg_feats code/mdl_conc_single.py:51-66)
__global__ void concat_rows_kernel(const float* a, int Na, int rep_a, const float* b, int Nb, int rep_b, float* out, int M) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = Na + Nb;
  if (i >= (int64_t)M * W) return;
  const int c = (int)(i % W);
  const int64_t m = i / W;
  out[i] = c < Na ? a[(m / rep_a) * Na + c] : b[(m / rep_b) * Nb + (c - Na)];
}
void concat_rows(const float* a, int Na, int rep_a, const float* b, int Nb, int rep_b, float* out, int M, hipStream_t st) {
  ::vog::launch(concat_rows_kernel, dim3((unsigned)(((int64_t)M * (Na + Nb) + 255) / 256)), dim3(256), 0, st, a, Na, rep_a, b, Nb, rep_b,
                out, M);
}

// x_mul[((q, v), f), (arg, p), :] = [ps[(q, v), f*nppf + p, :] | mask * lang[(q, v | 0), arg, :]]   (code/mdl_vog.py:316-344, 681-700)
__global__ void conc_fwd_kernel(const float* ps, const float* lang, const int64_t* mask, float* out, int n_q, int nc_v, int nfrm,
                                int nppf, int nsrl, int dobj, int dlang, int lang_per_vid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int vld = dobj + dlang;
  const int64_t total = (int64_t)n_q * nc_v * nfrm * nsrl * nppf * vld;
  if (i >= total) return;
  const int c = (int)(i % vld);
  int64_t r = i / vld;
  const int pp = (int)(r % nppf); r /= nppf;
  const int ar = (int)(r % nsrl); r /= nsrl;
  const int f = (int)(r % nfrm);
  const int64_t qv = r / nfrm;
  if (c < dobj) { out[i] = ps[((qv * nfrm + f) * nppf + pp) * dobj + c]; return; }
  const int64_t lr = (lang_per_vid ? qv : qv / nc_v) * nsrl + ar;
  out[i] = (mask && mask[lr] == 0) ? 0.f : lang[lr * dlang + (c - dobj)];
}

// mdl_outs[v, arg, f*nppf + p] = h[row] . w2 + b2, row = ((v, f), (arg, p))      (code/mdl_vog.py:224-230, 724-737)
__global__ __launch_bounds__(256) void score_fwd_kernel(const float* h, const float* w2, const float* b2, float* outs, int M, int HD,
                                                        int nfrm, int nppf, int nsrl) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  float s = 0.f;
  for (int i = lane; i < HD; i += 64) s += h[(int64_t)row * HD + i] * w2[i];
  s = wsum(s);
  if (lane == 0) {
    const int N = nsrl * nppf, sq = row / N, j = row % N, v = sq / nfrm, f = sq % nfrm, ar = j / nppf, pp = j % nppf;
    outs[((int64_t)v * nsrl + ar) * ((int64_t)nfrm * nppf) + (int64_t)f * nppf + pp] = s + b2[0];
  }
}

// out[g, n] = mean_f x[g, f, n]   (seg_feats.mean(dim=-2) of the sep verb head, code/mdl_conc_sep.py:64-129)
__global__ void row_mean_kernel(const float* x, float* out, int G, int F, int N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)G * N) return;
  const int n = (int)(i % N);
  const int64_t g = i / N;
  float s = 0.f;
  for (int f = 0; f < F; ++f) s += x[(g * F + f) * N + n];
  out[i] = s / (float)F;
}

// torch.optim.Adam (no weight decay, no amsgrad): the reference's optimizer, betas (0.9, 0.99) (code/main_dist.py:55)
__global__ void adam_kernel(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                            float bc1, float bc2_sqrt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  adam_update(p[i], g[i], m[i], v[i], lr, b1, b2, eps, bc1, bc2_sqrt);
}

}  // namespace vog

extern "C" int vog_concat_rows_f32(const float* a, int Na, int rep_a, const float* b, int Nb, int rep_b, float* out, int M, void* stream) {
  VOG_CHECK_ARG(a && b && out && Na > 0 && Nb > 0 && rep_a >= 1 && rep_b >= 1 && M > 0);
  concat_rows(a, Na, rep_a, b, Nb, rep_b, out, M, (hipStream_t)stream);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_conc_f32_fwd(const float* ps, const float* lang, const int64_t* inds_msk, float* out, int n_q, int nc_v, int nfrm,
                                int nppf, int nsrl, int dobj, int dlang, int lang_per_vid, void* stream) {
  VOG_CHECK_ARG(ps && lang && out && n_q > 0 && nc_v > 0 && nfrm > 0 && nppf > 0 && nsrl > 0 && dobj > 0 && dlang > 0);
  const int64_t total = (int64_t)n_q * nc_v * nfrm * nsrl * nppf * (dobj + dlang);
  ::vog::launch(conc_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ps, lang, inds_msk, out, n_q,
                nc_v, nfrm, nppf, nsrl, dobj, dlang, lang_per_vid);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_score_head_f32(const float* y, const float* wl, const float* bl, const float* wl2, const float* bl2, float* mdl_outs,
                                  void* scratch, size_t scratch_bytes, int M, int d, int dhead, int n_vid, int nfrm, int nppf, int nsrl,
                                  void* stream) {
  VOG_CHECK_ARG(y && wl && bl && wl2 && bl2 && mdl_outs && scratch && M > 0 && d > 0 && dhead > 0 && M == n_vid * nfrm * nppf * nsrl);
  if (scratch_bytes < (size_t)M * dhead * 4) VOG_FAIL(-2, "vog_score_head_f32: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  float* h = (float*)scratch;
  VOG_TRY(gemm_f32(y, d, 1, wl, 1, d, h, dhead, bl, 1, M, dhead, d, st));
  ::vog::launch(score_fwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, st, (const float*)h, wl2, bl2, mdl_outs, M, dhead, nfrm, nppf, nsrl);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                            int step, void* stream) {
  VOG_CHECK_ARG(p && g && m && v && n > 0 && step >= 1 && lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f);
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  ::vog::launch(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                bc1, sqrtf(bc2));
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_row_mean_f32(const float* x, float* out, int G, int F, int N, void* stream) {
  VOG_CHECK_ARG(x && out && G > 0 && F > 0 && N > 0);
  ::vog::launch(row_mean_kernel, dim3((unsigned)(((int64_t)G * N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, G, F, N);
  VOG_LAUNCH_CHECK();
  return 0;
}

// lin2 alone (ImgGrnd / VidGrnd: the score head reads the [vis | lang] token matrix directly, code/mdl_vog.py:224-230,
// 286-344): gradients of lin2.{0,2} and of its input. x [M, d], rows ((video, frame), (arg, p)) as vog_score_head_f32
// (frame-free models: nfrm = 1, nppf = NP).
struct ScoreHeadBufs { float *h, *dh, *hw, *dlog; ColPart part; int64_t bytes; };   // h, dh, hw [M, dhead]
static ScoreHeadBufs score_head_layout(void* base, int M, int dhead) {
  Carve c(base, 1, false);
  ScoreHeadBufs b;
  for (float** p : {&b.h, &b.dh, &b.hw}) *p = c.take<float>((int64_t)M * dhead);
  b.dlog = c.take<float>((M + 3) / 4 * 4);
  b.part = c.colpart(dhead);                           // hw, dh [M, dhead] and dlog [M, 1] are summed, nothing d wide
  b.bytes = c.bytes();
  return b;
}
extern "C" int64_t vog_score_head_f32_bwd_scratch_bytes(int M, int d, int dhead) {
  if (M <= 0 || d <= 0 || dhead <= 0) return -1;
  return score_head_layout(nullptr, M, dhead).bytes;
}
extern "C" int vog_score_head_f32_bwd(const float* x, const float* d_mdl_outs, const float* wl, const float* bl, const float* wl2,
                                      float* g_wl, float* g_bl, float* g_wl2, float* g_bl2, float* d_x, void* scratch,
                                      size_t scratch_bytes, int M, int d, int dhead, int n_vid, int nfrm, int nppf, int nsrl, void* stream) {
  VOG_CHECK_ARG(x && d_mdl_outs && wl && bl && wl2 && scratch && M == n_vid * nfrm * nppf * nsrl);   // (g_* / d_x: NULL = skipped)
  if ((int64_t)scratch_bytes < vog_score_head_f32_bwd_scratch_bytes(M, d, dhead)) VOG_FAIL(-2, "vog_score_head_f32_bwd: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const ScoreHeadBufs b = score_head_layout(scratch, M, dhead);
  float *h = b.h, *dh = b.dh, *hw = b.hw, *dlog = b.dlog;
  const ColPart part = b.part;
  VOG_TRY(gemm_f32(x, d, 1, wl, 1, d, h, dhead, bl, 1, M, dhead, d, st));
  ScoreBwd sb{d_mdl_outs, h, wl2, dh, hw, dlog, M, nfrm, nppf, nsrl, dhead};
  ::vog::launch(score_bwd_kernel, dim3(M), dim3(256), 0, st, sb);
  if (g_wl2) VOG_TRY(colsum(hw, g_wl2, part, M, dhead, st));
  if (g_bl2) VOG_TRY(colsum(dlog, g_bl2, part, M, 1, st));
  if (g_wl) VOG_TRY(gemm_f32(dh, 1, dhead, x, d, 1, g_wl, d, nullptr, 0, dhead, d, M, st));
  if (g_bl) VOG_TRY(colsum(dh, g_bl, part, M, dhead, st));
  if (d_x) VOG_TRY(gemm_f32(dh, dhead, 1, wl, d, 1, d_x, d, nullptr, 0, M, d, dhead, st));
  VOG_LAUNCH_CHECK();
  return 0;
}

// ---- the evaluation scores' backward and the gradient sums of the sep verb head's inputs ----
namespace vog {

// d_logits[o] = d_outs[o] + d_eval[o] * s (1 - s) * arg_msk * cmp_msk, s = sigmoid(logits[o]): the backward of
// mdl_outs_eval = sigmoid(mdl_outs) * masks with the masks broadcast as score_kernel (csrc/elementwise.hip) does;
// o = (v, arg, r) over [n_vid, nsrl, NP]
struct EvalBwd { const float* logits; const float* d_outs; const float* d_eval; const int64_t* arg_msk; const int64_t* cmp_msk;
                 float* d_logits; int64_t total; int nsrl, NP, conc_type, ncmp, nc_v, nvl, nfrm0, nppf0; };
__global__ void score_eval_bwd_kernel(EvalBwd a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.total) return;
  float g = a.d_outs ? a.d_outs[i] : 0.f;
  if (a.d_eval) {
    const int r = (int)(i % a.NP);
    const int64_t va = i / a.NP;
    const int arg = (int)(va % a.nsrl);
    const int v = (int)(va / a.nsrl);
    const int b = v / a.nc_v, c = v % a.nc_v;
    int cmp;
    if (a.conc_type == VOG_CONC_TEMP) cmp = r / (a.nfrm0 * a.nppf0);
    else if (a.conc_type == VOG_CONC_SPAT) cmp = (r / a.nppf0) % a.ncmp;
    else cmp = c;
    const int lrow = a.nvl > 1 ? (b * a.nvl + c) : b;
    const float m = (float)a.arg_msk[(int64_t)lrow * a.nsrl + arg] * (float)a.cmp_msk[(int64_t)b * a.ncmp + cmp];
    const float s = sigm(a.logits[i]);
    g += a.d_eval[i] * (s * (1.f - s)) * m;
  }
  a.d_logits[i] = g;
}

// out[m, c] = sum_{j < rep} x[(m*rep + j) * ldx + c] (+ y[(m / F) * ldy + c] / F)
__global__ void rep_sum_kernel(const float* x, int64_t ldx, int rep, const float* y, int64_t ldy, int F, float* out, int M, int N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int c = (int)(i % N);
  const int64_t m = i / N;
  float s = 0.f;
  for (int j = 0; j < rep; ++j) s += x[(m * rep + j) * ldx + c];
  if (y) s += y[(m / F) * ldy + c] / (float)F;
  out[i] = s;
}

}  // namespace vog

extern "C" int vog_score_eval_bwd_f32(const float* logits, const float* d_outs, const float* d_eval, const int64_t* arg_msk,
                                      const int64_t* cmp_msk, float* d_logits, int n_vid, int nsrl, int NP, int conc_type, int ncmp,
                                      int nc_v, int nvl, int nfrm0, int nppf0, void* stream) {
  VOG_CHECK_ARG(d_logits && n_vid > 0 && nsrl > 0 && NP > 0 && ncmp > 0 && nc_v > 0 && nfrm0 > 0 && nppf0 > 0);
  VOG_CHECK_ARG(n_vid % nc_v == 0 && (nvl == 1 || nvl == nc_v));
  if (d_eval) {
    VOG_CHECK_ARG(logits && arg_msk && cmp_msk);
    // the masks are indexed with the video / comparison of each proposal row: the geometry has to match the strategy
    if (conc_type == VOG_CONC_TEMP) VOG_CHECK_ARG(nc_v == 1 && NP == ncmp * nfrm0 * nppf0);
    else if (conc_type == VOG_CONC_SPAT) VOG_CHECK_ARG(nc_v == 1 && NP == nfrm0 * ncmp * nppf0);
    else VOG_CHECK_ARG(nc_v == ncmp);
  }
  const int64_t total = (int64_t)n_vid * nsrl * NP;
  EvalBwd a{logits, d_outs, d_eval, arg_msk, cmp_msk, d_logits, total, nsrl, NP, conc_type, ncmp, nc_v, nvl, nfrm0, nppf0};
  ::vog::launch(score_eval_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_rep_sum_f32(const float* x, int64_t ldx, int rep, const float* y, int64_t ldy, int F, float* out, int M, int N,
                               void* stream) {
  VOG_CHECK_ARG(x && out && rep >= 1 && M > 0 && N > 0 && ldx >= N && (!y || (F >= 1 && ldy >= N)));
  ::vog::launch(rep_sum_kernel, dim3((unsigned)(((int64_t)M * N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, rep, y, ldy,
                F > 0 ? F : 1, out, M, N);
  VOG_LAUNCH_CHECK();
  return 0;
}
