// Multi-tensor optimiser step of the training path (include/vog_hip.h: vog_opt_step_f32): torch.optim.Adam over a whole parameter
// set in a few launches, optionally with the gradient statistics in front of it that torch.amp.GradScaler (unscale, skip on a
// non-finite gradient, grow / back off the scale) and torch.nn.utils.clip_grad_norm_ need - decided on the device, nothing read
// back by the host. Beside it the passes over the same tables: gradient accumulation and weight averaging.
//
// Work is cut into CHUNKS of OPT_CHUNK elements of one tensor; a launch carries a table of tensors in its kernel arguments (the
// gradient pointers change every step, so a table in device memory would have to be uploaded per step anyway) and a grid of at
// most OPT_MAX_GRID workgroups that strides over the table's chunks in a fixed order. Inside a chunk the accesses are 16 bytes
// per lane wherever a tensor's pointers share their misalignment to 16 bytes (a scalar head of up to 3 elements brings them all
// to a boundary; a scalar tail ends the tensor); tensors whose pointers disagree run one element per lane. Every kernel takes
// this cut from ONE walk (opt_walk) and differs in what it does with an element.
#include <math.h>
#include "common.h"

namespace vog {

constexpr int OPT_THREADS = 256;
constexpr int OPT_UNROLL = 4;                                  // 16-byte accesses in flight per lane and array
constexpr int OPT_CHUNK = OPT_THREADS * 4 * OPT_UNROLL;        // elements per chunk (16 KiB of every array)
constexpr int OPT_MAX_GRID = 2048;                             // memory-bound: 256 CUs x 8 workgroups, the rest is strided
constexpr int OPT_HDR = 64;                                    // scratch: [bc1, bc2_sqrt, ...] then one float per statistics workgroup

// The launch table: K pointers per tensor (ptr[k][t]), at most CAP tensors. It must stay under vog::launch's 1 KiB record.
template <int K_, int CAP_>
struct OptTab {
  static constexpr int K = K_, CAP = CAP_;
  float* ptr[K_][CAP_];
  long long n[CAP_];
  int chunk0[CAP_ + 1];                                        // first chunk of tensor t; [n_tensors] = chunks of the launch
  int n_tensors;
};
enum { OPT_P = 0, OPT_G = 1, OPT_M = 2, OPT_V = 3, OPT_VMAX = 4 };   // the step's pointers
enum { OPT_DST = 0, OPT_SRC = 1 };                             // accumulation: acc, g; averaging: avg, p
constexpr int OPT_MAX_T = 20;                                  // tensors per launch of the step
using OptTable = OptTab<4, OPT_MAX_T>;
using OptTableV = OptTab<5, 16>;                               // with AMSGrad's vmax: 52 bytes per tensor, so fewer of them
using OptTable2 = OptTab<2, 32>;
static_assert(sizeof(OptTable) <= 960 && sizeof(OptTableV) <= 960 && sizeof(OptTable2) <= 960,
              "the tensor table and the scalars must fit a 1 KiB launch record");

// Elements in front of the first address at which all K pointers of tensor t are 16-byte aligned: 0..3, or -1 when they
// disagree (every pointer is 4-byte aligned: checked on the host).
template <typename Tab>
__host__ __device__ __forceinline__ int opt_tab_head(const Tab& tab, int t) {
  unsigned a[Tab::K];
#pragma unroll
  for (int k = 0; k < Tab::K; ++k) a[k] = (unsigned)(((uintptr_t)tab.ptr[k][t] >> 2) & 3);
#pragma unroll
  for (int k = 1; k < Tab::K; ++k)
    if (a[k] != a[0]) return -1;
  return (int)((4 - a[0]) & 3);
}
// Chunks of one tensor: chunk c covers [head + c * OPT_CHUNK, head + (c + 1) * OPT_CHUNK) of it, chunk 0 the head as well.
static inline int64_t opt_chunks(int64_t n, int head) {
  const int64_t body = n - (head > 0 ? (head < n ? head : n) : 0);
  return body <= 0 ? 1 : (body + OPT_CHUNK - 1) / OPT_CHUNK;
}

// The chunks of this workgroup, in ascending order (the tensor scan goes on from the last hit): elem(t, i) for every element
// that is handled alone (a tensor without a common alignment, heads, tails), vec(t, e0, n4) once per chunk for its n4 whole
// 16-byte groups from element e0 (16-byte aligned in every array of the table).
template <typename Tab, typename Elem, typename Vec>
__device__ __forceinline__ void opt_walk(const Tab& tab, Elem elem, Vec vec) {
  const int tid = threadIdx.x, total = tab.chunk0[tab.n_tensors];
  int t = 0;
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    while (t + 1 < tab.n_tensors && tab.chunk0[t + 1] <= c) ++t;
    const int64_t n = tab.n[t];
    const int cl = c - tab.chunk0[t];
    const int head = opt_tab_head(tab, t);
    if (head < 0) {
      const int64_t e0 = (int64_t)cl * OPT_CHUNK;
      for (int k = tid; k < OPT_CHUNK; k += OPT_THREADS) {
        const int64_t i = e0 + k;
        if (i < n) elem(t, i);
      }
      continue;
    }
    if (cl == 0 && tid < head && tid < n) elem(t, (int64_t)tid);
    const int64_t e0 = head + (int64_t)cl * OPT_CHUNK;
    const int64_t left = n - e0;
    const int n4 = (int)((left < OPT_CHUNK ? (left > 0 ? left : 0) : OPT_CHUNK) >> 2);
    vec(t, e0, n4);
    if (left > 0 && left < OPT_CHUNK && tid < (int)(left & 3)) elem(t, e0 + 4 * (int64_t)n4 + tid);
  }
}

// One element: adam_kernel's update (adam_update, common.h: the plain step must give its bits). `factor` = grad_scale x (mode
// B's coef), negated for MAXIMIZE: ONE multiplication of the gradient, by 1 in the plain mode-A step (exact: no fast-math, and
// the kernels keep fp32 denormals). DECAY: 0 none, 1 L2 (weight_decay * p joins the gradient behind the clipping, one fused
// multiply-add in adam_update, so it takes no part in the statistics), 2 decoupled (AdamW): p is multiplied by
// pmul = 1 - lr * wd (one rounding) in front of the moments and the gradient is left alone. AMS: vmax = max(vmax, v) feeds the
// denominator.
template <int DECAY, bool AMS>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, float lr, float b1, float b2, float eps,
                                          float bc1, float bc2_sqrt, float factor, float wd, float pmul) {
  if (DECAY == 2) p = p * pmul;
  if (AMS) adam_update_amsgrad<DECAY == 1>(p, g * factor, m, v, vmax, lr, b1, b2, eps, bc1, bc2_sqrt, wd);
  else adam_update<DECAY == 1>(p, g * factor, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, wd);
}

// The apply pass (Tab = OptTableV: AMSGrad). gscale = +-grad_scale. state == NULL (SCALED = false): bc1 / bc2_sqrt are the
// host's. SCALED: found_inf ends the kernel before anything is written; coef and the bias corrections of the step that is being
// applied are what opt_finalize_kernel left. lr, wd and pmul are those of the table's parameter group (a table never crosses a
// group boundary).
template <typename Tab, int DECAY>
__device__ __forceinline__ void opt_apply_body(const Tab& tab, float lr, float wd, float pmul, float b1, float b2, float eps, float bc1,
                                               float bc2_sqrt, float factor) {
  constexpr bool AMS = Tab::K == 5;
  const int tid = threadIdx.x;
  auto vmax_of = [&](int t) -> float* {
    if constexpr (AMS) return tab.ptr[OPT_VMAX][t]; else return nullptr;
  };
  opt_walk(tab,
    [&](int t, int64_t i) {
      float* vx = vmax_of(t);
      float vm = AMS ? vx[i] : 0.f;
      adam_elem<DECAY, AMS>(tab.ptr[OPT_P][t][i], tab.ptr[OPT_G][t][i], tab.ptr[OPT_M][t][i], tab.ptr[OPT_V][t][i], vm, lr, b1, b2, eps, bc1,
                            bc2_sqrt, factor, wd, pmul);
      if (AMS) vx[i] = vm;
    },
    [&](int t, int64_t e0, int n4) {
      float* p = tab.ptr[OPT_P][t] + e0;
      const float* g = tab.ptr[OPT_G][t] + e0;
      float* m = tab.ptr[OPT_M][t] + e0;
      float* v = tab.ptr[OPT_V][t] + e0;
      float* vx = AMS ? vmax_of(t) + e0 : nullptr;
      f32x4 P[OPT_UNROLL], G[OPT_UNROLL], M[OPT_UNROLL], V[OPT_UNROLL], X[OPT_UNROLL];
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) {
          G[u] = *reinterpret_cast<const f32x4*>(g + 4 * j);
          P[u] = *reinterpret_cast<const f32x4*>(p + 4 * j);
          M[u] = *reinterpret_cast<const f32x4*>(m + 4 * j);
          V[u] = *reinterpret_cast<const f32x4*>(v + 4 * j);
          if (AMS) X[u] = *reinterpret_cast<const f32x4*>(vx + 4 * j);
        }
      }
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float pp = P[u][q], mm = M[u][q], vv = V[u][q], xx = AMS ? X[u][q] : 0.f;
            adam_elem<DECAY, AMS>(pp, G[u][q], mm, vv, xx, lr, b1, b2, eps, bc1, bc2_sqrt, factor, wd, pmul);
            P[u][q] = pp; M[u][q] = mm; V[u][q] = vv;
            if (AMS) X[u][q] = xx;
          }
          *reinterpret_cast<f32x4*>(m + 4 * j) = M[u];
          *reinterpret_cast<f32x4*>(v + 4 * j) = V[u];
          if (AMS) *reinterpret_cast<f32x4*>(vx + 4 * j) = X[u];
          *reinterpret_cast<f32x4*>(p + 4 * j) = P[u];
        }
      }
    });
}

template <typename Tab, bool SCALED, int DECAY>
__global__ __launch_bounds__(OPT_THREADS) void opt_apply_kernel(Tab tab, float lr, float wd, float pmul, float b1, float b2, float eps,
                                                                float bc1, float bc2_sqrt, float gscale, const vog_opt_state* state,
                                                                const float* consts) {
  float factor = gscale;
  if (SCALED) {
    if (state->found_inf) return;
    factor = state->coef * gscale;
    bc1 = consts[0];
    bc2_sqrt = consts[1];
  }
  opt_apply_body<Tab, DECAY>(tab, lr, wd, pmul, b1, b2, eps, bc1, bc2_sqrt, factor);
}

// The apply pass WITHOUT per-step host scalars (vog_opt_step_dev_f32: a launch that a captured graph replays). lr is entry
// `group` of a device table; AdamW's factor is formed here from it as the host forms it, (float)(1.0 - (double)lr * (double)wd)
// (the product of two floats is exact in double: the same bits). Mode A (SCALED = false): the update's number is
// step->adam_step + 1 (vog_train_tick's VOG_TICK_END counts it behind the last apply launch) and its bias corrections are entry
// min(number, bias_len) - 1 of the host-built table (vog_opt_bias_table), whose last entry is (1, 1). Mode B is the host entry's.
template <typename Tab, bool SCALED, int DECAY>
__global__ __launch_bounds__(OPT_THREADS) void opt_apply_dev_kernel(Tab tab, const float* lr_tab, int group, float wd, float b1, float b2,
                                                                    float eps, float gscale, const vog_opt_state* state,
                                                                    const float* consts, const vog_train_step* step, const float* bias,
                                                                    int bias_len) {
  const float lr = lr_tab[group];
  const float pmul = DECAY == 2 ? (float)(1.0 - (double)lr * (double)wd) : 1.f;
  float factor = gscale, bc1, bc2_sqrt;
  if (SCALED) {
    if (state->found_inf) return;
    factor = state->coef * gscale;
    bc1 = consts[0];
    bc2_sqrt = consts[1];
  } else {
    const int s = step->adam_step + 1;
    const int i = (s < bias_len ? (s > 0 ? s : 1) : bias_len) - 1;
    bc1 = bias[2 * i];
    bc2_sqrt = bias[2 * i + 1];
  }
  opt_apply_body<Tab, DECAY>(tab, lr, wd, pmul, b1, b2, eps, bc1, bc2_sqrt, factor);
}

// Statistics: partial[blockIdx.x] = sum over this workgroup's chunks of (g * gscale / scale)^2 - with grad_scale folded into the
// division by the scale, the statistics see the AVERAGED gradient of an accumulation window (what clip_grad_norm_ would see),
// whatever its sign. Every lane adds its elements in a fixed order, the lanes are added in a fixed tree: no atomics, the same
// bits on every run and on every rank.
template <typename Tab>
__global__ __launch_bounds__(OPT_THREADS) void opt_stats_kernel(Tab tab, float gscale, const vog_opt_state* state, float* partial) {
  __shared__ float red[OPT_THREADS];
  const float inv = gscale / state->scale;
  const int tid = threadIdx.x;
  float acc = 0.f;
  opt_walk(tab,
    [&](int t, int64_t i) { const float x = tab.ptr[OPT_G][t][i] * inv; acc += x * x; },
    [&](int t, int64_t e0, int n4) {
      const float* g = tab.ptr[OPT_G][t] + e0;
      f32x4 G[OPT_UNROLL];
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) G[u] = *reinterpret_cast<const f32x4*>(g + 4 * j);
      }
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) {
#pragma unroll
          for (int q = 0; q < 4; ++q) { const float x = G[u][q] * inv; acc += x * x; }
        }
      }
    });
  red[tid] = acc;
  __syncthreads();
  for (int s = OPT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) partial[blockIdx.x] = red[0];
}

// Finalise (one workgroup): the partials in index order per lane, the lanes in a fixed tree, in double; then the decision of the
// step - torch.nn.utils.clip_grad_norm_'s coefficient, torch.amp.GradScaler.update's scale - written by lane 0.
__global__ __launch_bounds__(OPT_THREADS) void opt_finalize_kernel(const float* partial, int n_partial, vog_opt_state* state, float* consts,
                                                                   float b1, float b2, float max_norm, float growth_factor,
                                                                   float backoff_factor, int growth_interval) {
  __shared__ double red[OPT_THREADS];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n_partial; i += OPT_THREADS) acc += (double)partial[i];
  red[tid] = acc;
  __syncthreads();
  for (int s = OPT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid != 0) return;
  const double sum = red[0];
  const int found = !isfinite(sum);
  const float norm = (float)sqrt(sum);
  float scale = state->scale;
  int tracker = state->growth_tracker, step = state->adam_step;
  float clip = 1.f;
  if (max_norm > 0.f) { clip = max_norm / (norm + 1e-6f); clip = clip < 1.f ? clip : 1.f; }
  state->found_inf = found;
  state->grad_norm = norm;
  state->coef = found ? 0.f : clip / scale;
  if (found) {
    if (growth_interval > 0) scale *= backoff_factor;
    tracker = 0;
    state->skipped += 1;
  } else {
    step += 1;
    tracker += 1;
    if (growth_interval > 0 && tracker >= growth_interval) { scale *= growth_factor; tracker = 0; }
  }
  state->scale = scale;
  state->growth_tracker = tracker;
  state->adam_step = step;
  const int s1 = step > 0 ? step : 1;                           // (a skipped first step applies nothing: any finite value)
  consts[0] = 1.f - powf(b1, (float)s1);
  consts[1] = sqrtf(1.f - powf(b2, (float)s1));
}

// x *= state->scale: 16 bytes per lane from the first aligned address, workgroup 0 takes the head and the tail
__global__ __launch_bounds__(OPT_THREADS) void opt_scale_kernel(float* x, int64_t n, const vog_opt_state* state) {
  const float s = state->scale;
  const int64_t h0 = (int64_t)((4 - (((uintptr_t)x >> 2) & 3)) & 3);
  const int64_t head = h0 < n ? h0 : n;
  const int64_t n4 = (n - head) >> 2;
  for (int64_t j = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; j < n4; j += (int64_t)gridDim.x * OPT_THREADS) {
    f32x4* q = reinterpret_cast<f32x4*>(x + head + 4 * j);
    f32x4 val = *q;
    val *= s;
    *q = val;
  }
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + 4 * n4;
    if (threadIdx.x < head) x[threadIdx.x] *= s;
    else if (threadIdx.x >= 64 && tail0 + (threadIdx.x - 64) < n) x[tail0 + (threadIdx.x - 64)] *= s;
  }
}

// Gradient accumulation (vog_opt_accum_f32). acc[i] += g[i]: every element is read, added once and written by one lane - no
// atomics, one rounding.
__global__ __launch_bounds__(OPT_THREADS) void opt_accum_kernel(OptTable2 tab) {
  const int tid = threadIdx.x;
  opt_walk(tab,
    [&](int t, int64_t i) { tab.ptr[OPT_DST][t][i] += tab.ptr[OPT_SRC][t][i]; },
    [&](int t, int64_t e0, int n4) {
      float* a = tab.ptr[OPT_DST][t] + e0;
      const float* g = tab.ptr[OPT_SRC][t] + e0;
      f32x4 A[OPT_UNROLL], G[OPT_UNROLL];
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) {
          G[u] = *reinterpret_cast<const f32x4*>(g + 4 * j);
          A[u] = *reinterpret_cast<const f32x4*>(a + 4 * j);
        }
      }
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) *reinterpret_cast<f32x4*>(a + 4 * j) = A[u] + G[u];
      }
    });
}

// ---- weight averaging (vog_opt_average_f32): EMA / SWA of the parameters behind the optimiser step ------------------------------
// Two launches' worth of code: ONE decision (a single workgroup, lane 0) that turns the step count and the optimiser's found_inf
// into the interpolation weight of this call, left in the caller's state block, and the apply pass that reads it. Nothing is
// read back by the host; mode A (host-counted step) and mode B (the optimiser's device block) share the path.

// The weight of this call: w = 0 (skip) | 1 (the first update: a copy) | 1 / (n + 1) (SWA) | 1 - decay_eff (EMA), formed in
// double and rounded once (opt_launch_apply's pmul convention). torch.optim.swa_utils.AveragedModel's lerp weights.
// ts (vog_opt_average_dev_f32, mode A of a captured step): the count is the update just applied, ts->adam_step + 1.
__global__ __launch_bounds__(64) void opt_avg_decide_kernel(vog_opt_avg_state* state, const vog_opt_state* opt_state, int step, int mode,
                                                           double decay, int warmup, int start, int every, const vog_train_step* ts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int s = opt_state ? opt_state->adam_step : (ts ? ts->adam_step + 1 : step);
  const bool skip = (opt_state && opt_state->found_inf) || s < start || (s - start) % every != 0;
  if (skip) {
    state->updated = 0;
    state->w = 0.f;
    return;
  }
  const int n = state->n_averaged;
  double w = 1.0;
  if (n > 0) {
    if (mode == VOG_AVG_SWA) {
      w = 1.0 / ((double)n + 1.0);
    } else {
      double d = decay;
      if (warmup) { const double dw = (1.0 + (double)n) / (10.0 + (double)n); d = d < dw ? d : dw; }
      w = 1.0 - d;
    }
  }
  state->n_averaged = n + 1;
  state->updated = 1;
  state->w = (float)w;
}

// avg = lerp(avg, p, w) = fma(w, p - avg, avg); w == 1 stores p's bits, w == 0 touches nothing. Every element is written by one
// lane: no atomics, the same bits on every run and every rank.
__global__ __launch_bounds__(OPT_THREADS) void opt_avg_kernel(OptTable2 tab, const vog_opt_avg_state* state) {
  const float w = state->w;
  if (w == 0.f) return;
  const bool copy = w == 1.f;
  const int tid = threadIdx.x;
  opt_walk(tab,
    [&](int t, int64_t i) {
      const float x = tab.ptr[OPT_SRC][t][i];
      tab.ptr[OPT_DST][t][i] = copy ? x : fmaf(w, x - tab.ptr[OPT_DST][t][i], tab.ptr[OPT_DST][t][i]);
    },
    [&](int t, int64_t e0, int n4) {
      float* a = tab.ptr[OPT_DST][t] + e0;
      const float* p = tab.ptr[OPT_SRC][t] + e0;
      f32x4 A[OPT_UNROLL], P[OPT_UNROLL];
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) {
          P[u] = *reinterpret_cast<const f32x4*>(p + 4 * j);
          if (!copy) A[u] = *reinterpret_cast<const f32x4*>(a + 4 * j);
        }
      }
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int j = u * OPT_THREADS + tid;
        if (j < n4) {
          f32x4 R = P[u];
          if (!copy) {
#pragma unroll
            for (int q = 0; q < 4; ++q) R[q] = fmaf(w, P[u][q] - A[u][q], A[u][q]);
          }
          *reinterpret_cast<f32x4*>(a + 4 * j) = R;
        }
      }
    });
}

static int64_t opt_partial_slots(int n_tensors, int64_t total_elems) {
  const int64_t groups = (n_tensors + OPT_MAX_T - 1) / OPT_MAX_T;
  const int64_t by_grid = groups * OPT_MAX_GRID, by_work = total_elems / OPT_CHUNK + n_tensors;
  return by_grid < by_work ? by_grid : by_work;
}

}  // namespace vog

extern "C" int64_t vog_opt_scratch_bytes(int n_tensors, int64_t total_elems) {
  if (n_tensors <= 0 || total_elems <= 0) return ::vog::OPT_HDR;
  return ::vog::OPT_HDR + 4 * ::vog::opt_partial_slots(n_tensors, total_elems);
}

namespace vog {

// One launch: a table and its grids. lr and wd are those of the step's parameter group (the two-pointer passes leave them 0).
template <typename Tab>
struct OptLaunch { Tab tab; int grid, stats_grid; float lr, wd; int group; };   // grid: apply; stats_grid: statistics (one partial each)

// Tensors [first, first + count) cut into launches after a table's worth of them, in the caller's order, appended to `ls`.
// fill(i, ptr) stores the K pointers of tensor i and returns its length.
template <typename Tab, typename Fill>
static int opt_tables(int first, int count, float lr, float wd, Fill fill, std::vector<OptLaunch<Tab>>& ls, int group = 0) {
  constexpr int cap = Tab::CAP;
  for (int i0 = first; i0 < first + count; i0 += cap) {
    OptLaunch<Tab> l;
    memset(&l, 0, sizeof(l));
    Tab& tab = l.tab;
    const int left = first + count - i0;
    tab.n_tensors = left < cap ? left : cap;
    int64_t chunks = 0;
    for (int j = 0; j < tab.n_tensors; ++j) {
      float* ptr[Tab::K];
      tab.n[j] = fill(i0 + j, ptr);
      for (int k = 0; k < Tab::K; ++k) tab.ptr[k][j] = ptr[k];
      tab.chunk0[j] = (int)chunks;
      chunks += opt_chunks(tab.n[j], opt_tab_head(tab, j));
      VOG_CHECK_ARG(chunks < ((int64_t)1 << 31));
    }
    tab.chunk0[tab.n_tensors] = (int)chunks;
    l.grid = l.stats_grid = (int)(chunks < OPT_MAX_GRID ? chunks : OPT_MAX_GRID);
    l.lr = lr;
    l.wd = wd;
    l.group = group;
    ls.push_back(l);
  }
  return 0;
}

// The per-tensor checks of the two-pointer entries (accumulation, averaging)
static int opt_check_pair(const char* who, int i, const void* dst, const void* src, int64_t n) {
  if (!dst || !src) VOG_FAIL(-1, "%s: tensor %d has a NULL pointer", who, i);
  if (n <= 0 || n >= ((int64_t)1 << 40)) VOG_FAIL(-1, "%s: tensor %d has n = %lld", who, i, (long long)n);
  if (((uintptr_t)dst | (uintptr_t)src) & 3) VOG_FAIL(-1, "%s: tensor %d is not 4-byte aligned", who, i);
  return 0;
}

// What vog_opt_step_ex_f32 adds to a grouped step ({0, NULL, 1}: the plain step)
struct OptEx { unsigned flags; float* const* vmax; float grad_scale; };

// Argument checks of a step, before any launch -> the tensors and elements the groups cover. Tensors outside every group are
// in no table: not validated, not measured, not touched.
static int opt_check_groups(const vog_opt_args* a, const vog_opt_group* groups, int n_groups, const OptEx& ex, const char* who,
                            int* covered_out, int64_t* total_out, bool dev_step = false) {
  VOG_CHECK_ARG(a && a->tensors && a->n_tensors > 0);
  VOG_CHECK_ARG(groups && n_groups > 0);
  VOG_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f);
  const bool ams = (ex.flags & VOG_OPT_AMSGRAD) != 0;
  if (ex.flags & ~(unsigned)(VOG_OPT_DECOUPLED | VOG_OPT_AMSGRAD | VOG_OPT_MAXIMIZE))
    VOG_FAIL(-1, "%s: unknown flag bits 0x%x", who, ex.flags & ~(unsigned)(VOG_OPT_DECOUPLED | VOG_OPT_AMSGRAD | VOG_OPT_MAXIMIZE));
  if (!(ex.grad_scale > 0.f && isfinite(ex.grad_scale))) VOG_FAIL(-1, "%s: grad_scale = %g, a positive finite number", who, (double)ex.grad_scale);
  if (ams && !ex.vmax) VOG_FAIL(-1, "%s: VOG_OPT_AMSGRAD without the vmax table", who);
  int64_t total = 0;
  int covered = 0, next = 0;
  for (int k = 0; k < n_groups; ++k) {
    const vog_opt_group& gr = groups[k];
    if (gr.count <= 0) VOG_FAIL(-1, "%s: group %d is empty (count %d)", who, k, gr.count);
    if (gr.first < next) VOG_FAIL(-1, "%s: group %d starts at tensor %d, before %d: groups are disjoint and ascending", who, k, gr.first, next);
    if ((int64_t)gr.first + gr.count > a->n_tensors)
      VOG_FAIL(-1, "%s: group %d covers tensors [%d, %lld), the table has %d", who, k, gr.first, (long long)gr.first + gr.count, a->n_tensors);
    VOG_CHECK_ARG(gr.lr >= 0.f && gr.weight_decay >= 0.f && isfinite(gr.lr) && isfinite(gr.weight_decay));
    next = gr.first + gr.count;
    covered += gr.count;
    for (int i = gr.first; i < next; ++i) {
      const vog_opt_tensor& t = a->tensors[i];
      VOG_CHECK_ARG(t.p && t.g && t.m && t.v && t.n > 0 && t.n < ((int64_t)1 << 40));
      VOG_CHECK_ARG((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3) == 0);
      if (ams) {
        if (!ex.vmax[i]) VOG_FAIL(-1, "%s: vmax[%d] is NULL (tensor %d is in group %d)", who, i, i, k);
        if (((uintptr_t)ex.vmax[i]) & 3) VOG_FAIL(-1, "%s: vmax[%d] is not 4-byte aligned", who, i);
      }
      total += t.n;
    }
  }
  const bool scaled = a->state != nullptr;
  if (!scaled && !dev_step) VOG_CHECK_ARG(a->step >= 1);          // (the device-counted step reads vog_train_step.adam_step)
  if (scaled) {
    VOG_CHECK_ARG(a->growth_interval <= 0 || (a->growth_factor >= 1.f && a->backoff_factor > 0.f && a->backoff_factor <= 1.f));
    VOG_CHECK_ARG(a->scratch && (((uintptr_t)a->scratch) & 7) == 0);
    if ((int64_t)a->scratch_bytes < vog_opt_scratch_bytes(covered, total))
      VOG_FAIL(-2, "%s: scratch of %zu bytes, vog_opt_scratch_bytes(%d, %lld) = %lld", who, a->scratch_bytes, covered,
               (long long)total, (long long)vog_opt_scratch_bytes(covered, total));
  }
  *covered_out = covered;
  *total_out = total;
  return 0;
}

// One partial per statistics workgroup, within what vog_opt_scratch_bytes promised: tables cut at group boundaries (or smaller
// tables) can be more than ceil(n / OPT_MAX_T), and then every STATISTICS grid gets an equal share of the bound (never with one
// group of full tables: those grids fit); the apply launches keep their full grids
template <typename Tab>
static int opt_fit_stats(std::vector<OptLaunch<Tab>>& ls, int covered, int64_t total, const char* who) {
  int64_t slots = 0;
  for (size_t k = 0; k < ls.size(); ++k) slots += ls[k].stats_grid;
  const int64_t bound = opt_partial_slots(covered, total);
  if (slots > bound) {
    const int64_t cap = bound / (int64_t)ls.size();
    if (cap < 1) VOG_FAIL(-3, "%s: partial count exceeds the scratch bound", who);
    slots = 0;
    for (size_t k = 0; k < ls.size(); ++k) {
      if (ls[k].stats_grid > cap) ls[k].stats_grid = (int)cap;
      slots += ls[k].stats_grid;
    }
  }
  if (slots > bound) VOG_FAIL(-3, "%s: partial count exceeds the scratch bound", who);
  return 0;
}

// One apply launch: the DECAY instance of the table's group
template <typename Tab, bool SCALED>
static void opt_launch_apply(const OptLaunch<Tab>& l, const vog_opt_args* a, bool decoupled, float bc1, float bc2_sqrt, float gscale,
                             const float* consts, hipStream_t st) {
  // decoupled: p *= 1 - lr * wd, the factor rounded once from the double product (torch forms it in double)
  const float pmul = (float)(1.0 - (double)l.lr * (double)l.wd);
  const dim3 grid((unsigned)l.grid), block(OPT_THREADS);
  const vog_opt_state* state = (const vog_opt_state*)a->state;
  if (l.wd == 0.f)
    ::vog::launch(opt_apply_kernel<Tab, SCALED, 0>, grid, block, 0, st, l.tab, l.lr, 0.f, 1.f, a->beta1, a->beta2, a->eps, bc1, bc2_sqrt,
                  gscale, state, consts);
  else if (decoupled)
    ::vog::launch(opt_apply_kernel<Tab, SCALED, 2>, grid, block, 0, st, l.tab, l.lr, l.wd, pmul, a->beta1, a->beta2, a->eps, bc1, bc2_sqrt,
                  gscale, state, consts);
  else
    ::vog::launch(opt_apply_kernel<Tab, SCALED, 1>, grid, block, 0, st, l.tab, l.lr, l.wd, 1.f, a->beta1, a->beta2, a->eps, bc1, bc2_sqrt,
                  gscale, state, consts);
}

// The device-table form of one apply launch (vog_opt_dev_args)
template <typename Tab, bool SCALED>
static void opt_launch_apply_dev(const OptLaunch<Tab>& l, const vog_opt_args* a, bool decoupled, float gscale, const float* consts,
                                 const vog_opt_dev_args* dv, hipStream_t st) {
  const dim3 grid((unsigned)l.grid), block(OPT_THREADS);
  const vog_opt_state* state = (const vog_opt_state*)a->state;
  auto go = [&](auto kern, float wd) {
    ::vog::launch(kern, grid, block, 0, st, l.tab, dv->lr, l.group, wd, a->beta1, a->beta2, a->eps, gscale, state, consts, dv->step, dv->bias,
                  dv->bias_len);
  };
  if (l.wd == 0.f) go(opt_apply_dev_kernel<Tab, SCALED, 0>, 0.f);
  else if (decoupled) go(opt_apply_dev_kernel<Tab, SCALED, 2>, l.wd);
  else go(opt_apply_dev_kernel<Tab, SCALED, 1>, l.wd);
}

// The step over the tensors the groups cover (`who` names the entry in messages; Tab = OptTableV with VOG_OPT_AMSGRAD): the
// checks, the tables - cut at group boundaries - and then mode A's apply launches, or mode B's statistics, finalise and apply.
template <typename Tab>
static int opt_step(const vog_opt_args* a, const vog_opt_group* groups, int n_groups, const OptEx& ex, const char* who, void* stream,
                    const vog_opt_dev_args* dv = nullptr) {
  int covered = 0;
  int64_t total = 0;
  if (int rc = opt_check_groups(a, groups, n_groups, ex, who, &covered, &total, dv != nullptr)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool decoupled = (ex.flags & VOG_OPT_DECOUPLED) != 0;
  const float gscale = (ex.flags & VOG_OPT_MAXIMIZE) ? -ex.grad_scale : ex.grad_scale;
  std::vector<OptLaunch<Tab>> ls;
  for (int k = 0; k < n_groups; ++k) {
    const vog_opt_group& gr = groups[k];
    auto fill = [&](int i, float** ptr) {
      const vog_opt_tensor& t = a->tensors[i];
      ptr[OPT_P] = t.p; ptr[OPT_G] = const_cast<float*>(t.g); ptr[OPT_M] = t.m; ptr[OPT_V] = t.v;
      if constexpr (Tab::K == 5) ptr[OPT_VMAX] = ex.vmax[i];
      return t.n;
    };
    if (int rc = opt_tables<Tab>(gr.first, gr.count, gr.lr, gr.weight_decay, fill, ls, k)) return rc;
  }
  if (!a->state && dv) {                                      // mode A, counted on the device
    for (size_t k = 0; k < ls.size(); ++k) {
      opt_launch_apply_dev<Tab, false>(ls[k], a, decoupled, gscale, (const float*)nullptr, dv, st);
      VOG_LAUNCH_CHECK();
    }
    return 0;
  }
  if (!a->state) {
    const float bc1 = 1.f - powf(a->beta1, (float)a->step), bc2 = 1.f - powf(a->beta2, (float)a->step);
    for (size_t k = 0; k < ls.size(); ++k) {
      opt_launch_apply<Tab, false>(ls[k], a, decoupled, bc1, sqrtf(bc2), gscale, (const float*)nullptr, st);
      VOG_LAUNCH_CHECK();
    }
    return 0;
  }
  if (int rc = opt_fit_stats(ls, covered, total, who)) return rc;
  float* consts = (float*)a->scratch;
  float* partial = (float*)((char*)a->scratch + OPT_HDR);
  int n_partial = 0;
  for (size_t k = 0; k < ls.size(); ++k) {
    ::vog::launch(opt_stats_kernel<Tab>, dim3((unsigned)ls[k].stats_grid), dim3(OPT_THREADS), 0, st, ls[k].tab, ex.grad_scale,
                  (const vog_opt_state*)a->state, partial + n_partial);
    VOG_LAUNCH_CHECK();
    n_partial += ls[k].stats_grid;
  }
  ::vog::launch(opt_finalize_kernel, dim3(1), dim3(OPT_THREADS), 0, st, (const float*)partial, n_partial, a->state, consts, a->beta1,
                a->beta2, a->max_norm, a->growth_factor, a->backoff_factor, a->growth_interval);
  VOG_LAUNCH_CHECK();
  for (size_t k = 0; k < ls.size(); ++k) {
    if (dv) opt_launch_apply_dev<Tab, true>(ls[k], a, decoupled, gscale, (const float*)consts, dv, st);
    else opt_launch_apply<Tab, true>(ls[k], a, decoupled, 1.f, 1.f, gscale, (const float*)consts, st);
    VOG_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace vog

// One group over every tensor, at a->lr, without decay.
extern "C" int vog_opt_step_f32(const vog_opt_args* a, void* stream) {
  VOG_CHECK_ARG(a && a->tensors && a->n_tensors > 0);
  VOG_CHECK_ARG(a->lr >= 0.f);
  const vog_opt_group all = {0, a->n_tensors, a->lr, 0.f};
  return ::vog::opt_step<::vog::OptTable>(a, &all, 1, {0u, nullptr, 1.f}, "vog_opt_step_f32", stream);
}

extern "C" int vog_opt_step_groups_f32(const vog_opt_groups_args* a, void* stream) {
  VOG_CHECK_ARG(a && a->groups && a->n_groups > 0);
  return ::vog::opt_step<::vog::OptTable>(&a->base, a->groups, a->n_groups, {0u, nullptr, 1.f}, "vog_opt_step_groups_f32", stream);
}

// flags == 0 and grad_scale == 1 is the grouped step itself: the same kernels with the same arguments, hence the same bits.
extern "C" int vog_opt_step_ex_f32(const vog_opt_ex_args* a, void* stream) {
  using namespace ::vog;
  const char* who = "vog_opt_step_ex_f32";
  VOG_CHECK_ARG(a && a->groups.groups && a->groups.n_groups > 0);
  const OptEx ex = {a->flags, a->vmax, a->grad_scale};
  if (ex.flags & VOG_OPT_AMSGRAD) return opt_step<OptTableV>(&a->groups.base, a->groups.groups, a->groups.n_groups, ex, who, stream);
  return opt_step<OptTable>(&a->groups.base, a->groups.groups, a->groups.n_groups, ex, who, stream);
}

// The grouped step without per-step host scalars: every launch reads lr (and, in mode A, the update's number and its bias
// corrections) from device memory, so a captured graph can replay it. groups[k].lr is not read: d->lr[k] is.
extern "C" int vog_opt_step_dev_f32(const vog_opt_ex_args* a, const vog_opt_dev_args* d, void* stream) {
  using namespace ::vog;
  const char* who = "vog_opt_step_dev_f32";
  VOG_CHECK_ARG(a && a->groups.groups && a->groups.n_groups > 0);
  VOG_CHECK_ARG(d && d->lr && (((uintptr_t)d->lr) & 3) == 0);
  if (!a->groups.base.state) {
    if (!d->step || !d->bias || d->bias_len < 1) VOG_FAIL(-1, "%s: mode A needs the step block and the bias table (vog_opt_bias_table)", who);
    VOG_CHECK_ARG(((((uintptr_t)d->step) & 7) | (((uintptr_t)d->bias) & 3)) == 0);
  }
  const OptEx ex = {a->flags, a->vmax, a->grad_scale};
  if (ex.flags & VOG_OPT_AMSGRAD) return opt_step<OptTableV>(&a->groups.base, a->groups.groups, a->groups.n_groups, ex, who, stream, d);
  return opt_step<OptTable>(&a->groups.base, a->groups.groups, a->groups.n_groups, ex, who, stream, d);
}

// HOST function: mode A's bias corrections of update s = 1, 2, ... by the expressions of opt_step above, as (bc1, bc2_sqrt)
// pairs, up to and including the first s where both are 1.0f (from there they stay 1.0f). *len = that s; -2 when it passes cap
// (out then holds the first cap entries), also when it passes 2^20.
extern "C" int vog_opt_bias_table(float beta1, float beta2, float* out, int cap, int* len) {
  using namespace ::vog;
  VOG_CHECK_ARG(len && cap >= 0 && (out || cap == 0));
  VOG_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f);
  const int limit = 1 << 20;
  int s = 1;
  for (;; ++s) {
    const float bc1 = 1.f - powf(beta1, (float)s), bc2 = 1.f - powf(beta2, (float)s);
    const float bc2_sqrt = sqrtf(bc2);
    if (s <= cap) { out[2 * (s - 1)] = bc1; out[2 * (s - 1) + 1] = bc2_sqrt; }
    if (bc1 == 1.f && bc2_sqrt == 1.f) break;
    if (s > limit) { *len = s; VOG_FAIL(-2, "vog_opt_bias_table: betas (%g, %g) need more than 2^20 entries", (double)beta1, (double)beta2); }
  }
  *len = s;
  if (s > cap) VOG_FAIL(-2, "vog_opt_bias_table: %d entries, the table holds %d", s, cap);
  return 0;
}

extern "C" int vog_opt_accum_f32(const vog_opt_accum_tensor* tensors, int n_tensors, void* stream) {
  using namespace ::vog;
  VOG_CHECK_ARG(tensors && n_tensors > 0);
  for (int i = 0; i < n_tensors; ++i)
    if (int rc = opt_check_pair("vog_opt_accum_f32", i, tensors[i].acc, tensors[i].g, tensors[i].n)) return rc;
  std::vector<OptLaunch<OptTable2>> ls;
  auto fill = [&](int i, float** ptr) {
    ptr[OPT_DST] = tensors[i].acc; ptr[OPT_SRC] = const_cast<float*>(tensors[i].g);
    return tensors[i].n;
  };
  if (int rc = opt_tables<OptTable2>(0, n_tensors, 0.f, 0.f, fill, ls)) return rc;
  for (size_t k = 0; k < ls.size(); ++k) {
    ::vog::launch(opt_accum_kernel, dim3((unsigned)ls[k].grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, ls[k].tab);
    VOG_LAUNCH_CHECK();
  }
  return 0;
}

namespace vog { static int opt_average(const vog_opt_avg_args* a, const vog_train_step* ts, const char* who, void* stream); }
extern "C" int vog_opt_average_f32(const vog_opt_avg_args* a, void* stream) {
  return ::vog::opt_average(a, nullptr, "vog_opt_average_f32", stream);
}
// Mode A with the step from the device block (a->step is not read); with a->opt_state it is vog_opt_average_f32.
extern "C" int vog_opt_average_dev_f32(const vog_opt_avg_args* a, const vog_train_step* step, void* stream) {
  VOG_CHECK_ARG(a && (a->opt_state || (step && (((uintptr_t)step) & 7) == 0)));
  return ::vog::opt_average(a, a->opt_state ? nullptr : step, "vog_opt_average_dev_f32", stream);
}
static int vog::opt_average(const vog_opt_avg_args* a, const vog_train_step* ts, const char* who, void* stream) {
  VOG_CHECK_ARG(a && a->tensors && a->n_tensors > 0);
  if (a->mode != VOG_AVG_EMA && a->mode != VOG_AVG_SWA) VOG_FAIL(-1, "%s: mode = %d, VOG_AVG_EMA (1) or VOG_AVG_SWA (2)", who, a->mode);
  if (a->mode == VOG_AVG_EMA && !(a->decay >= 0.0 && a->decay <= 1.0)) VOG_FAIL(-1, "%s: decay = %g, a number in [0, 1]", who, a->decay);
  if (a->start < 1 || a->every < 1) VOG_FAIL(-1, "%s: start = %d, every = %d: both are >= 1", who, a->start, a->every);
  if (!a->opt_state && !ts && a->step < 1) VOG_FAIL(-1, "%s: step = %d without opt_state (mode A counts applied steps from 1)", who, a->step);
  if (!a->state) VOG_FAIL(-1, "%s: state is NULL", who);
  if (((uintptr_t)a->state | (uintptr_t)a->opt_state) & 3) VOG_FAIL(-1, "%s: state / opt_state is not 4-byte aligned", who);
  for (int i = 0; i < a->n_tensors; ++i)
    if (int rc = opt_check_pair(who, i, a->tensors[i].avg, a->tensors[i].p, a->tensors[i].n)) return rc;
  std::vector<OptLaunch<OptTable2>> ls;
  auto fill = [&](int i, float** ptr) {
    ptr[OPT_DST] = a->tensors[i].avg; ptr[OPT_SRC] = const_cast<float*>(a->tensors[i].p);
    return a->tensors[i].n;
  };
  if (int rc = opt_tables<OptTable2>(0, a->n_tensors, 0.f, 0.f, fill, ls)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ::vog::launch(opt_avg_decide_kernel, dim3(1), dim3(64), 0, st, a->state, a->opt_state, a->step, a->mode, a->decay, a->warmup, a->start,
                a->every, ts);
  VOG_LAUNCH_CHECK();
  for (size_t k = 0; k < ls.size(); ++k) {
    ::vog::launch(opt_avg_kernel, dim3((unsigned)ls[k].grid), dim3(OPT_THREADS), 0, st, ls[k].tab, (const vog_opt_avg_state*)a->state);
    VOG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int vog_opt_scale_grad_f32(float* x, int64_t n, const vog_opt_state* state, void* stream) {
  using namespace ::vog;
  VOG_CHECK_ARG(x && n > 0 && state && (((uintptr_t)x) & 3) == 0);
  const int64_t blocks = (n / 4 + OPT_THREADS - 1) / OPT_THREADS;
  const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks < OPT_MAX_GRID ? blocks : OPT_MAX_GRID));
  ::vog::launch(opt_scale_kernel, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, x, n, state);
  VOG_LAUNCH_CHECK();
  return 0;
}
