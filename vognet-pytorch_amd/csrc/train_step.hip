// The device step block of a CAPTURED training iteration (include/vog_hip.h: vog_train_step, vog_train_tick). A replayed graph
// cannot take per-step values from kernel arguments, so what changes from step to step lives here, in device memory the caller
// owns: the iteration count (numbers the dropout masks: train_dev.h::Drop.tick), the count of applied plain-Adam updates (the
// bias corrections of optim.hip's device-counted step) and a sticky word for sentence lengths that had to be clamped.
//
// One launch per phase, one workgroup: VOG_TICK_BEGIN runs as the first node of the step (the length guard), VOG_TICK_END as
// its last (the loss log, then the counts). Every word is written by one lane with an ordinary vector store - no atomics.
#include "common.h"

namespace vog {

constexpr int TICK_THREADS = 256;

// lens[i] = min(lens[i], T) and cap[i] = min(max(cap[i], 0), T - 1) in place (cap: the positions the argument vectors are
// gathered from, which index the T rows of a sentence); the sticky word is stored only when a value had to move
__global__ __launch_bounds__(TICK_THREADS) void train_tick_begin_kernel(vog_train_step* step, long long* lens, int n_lens, int T,
                                                                        long long* cap, int n_cap) {
  __shared__ int any;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  bool over = false;
  for (int i = threadIdx.x; i < n_lens; i += TICK_THREADS)
    if (lens[i] > (long long)T) { lens[i] = (long long)T; over = true; }
  for (int i = threadIdx.x; i < n_cap; i += TICK_THREADS) {
    const long long c = cap[i];
    if (c >= (long long)T) { cap[i] = (long long)T - 1; over = true; }
    else if (c < 0) { cap[i] = 0; over = true; }
  }
  if (over) any = 1;                                    // (every writer stores the same value)
  __syncthreads();
  if (threadIdx.x == 0 && any) step->len_clamped = 1;
}

// row tick % log_rows of the ring = [n_loss values | marker = the low 32 bits of tick + 1], this step's row only; then the counts
__global__ __launch_bounds__(64) void train_tick_end_kernel(vog_train_step* step, const float* loss_src, float* loss_log, int log_rows,
                                                           int n_loss, int count_adam) {
  const long long tick = step->tick;
  if (loss_log) {
    float* row = loss_log + (tick % (long long)log_rows) * (long long)(n_loss + 1);
    if ((int)threadIdx.x < n_loss) row[threadIdx.x] = loss_src[threadIdx.x];
    if ((int)threadIdx.x == n_loss) reinterpret_cast<unsigned int*>(row)[n_loss] = (unsigned int)((unsigned long long)tick + 1ull);
  }
  __syncthreads();                                      // (every lane has read the tick)
  if (threadIdx.x == 0) {
    step->tick = tick + 1;
    if (count_adam) step->adam_step += 1;
  }
}

}  // namespace vog

// The number of nodes of a captured graph (hipGraph_t), for records of what a captured step holds.
extern "C" int vog_graph_node_count(void* graph, int* n) {
  VOG_CHECK_ARG(graph && n);
  size_t count = 0;
  VOG_HIP(hipGraphGetNodes((hipGraph_t)graph, nullptr, &count));
  *n = (int)count;
  return 0;
}

extern "C" int vog_train_tick(vog_train_step* step, int64_t* lens, int n_lens, int T, const float* loss_src, float* loss_log,
                              int log_rows, int n_loss, int phase, int count_adam, int64_t* capture, int n_capture, void* stream) {
  using namespace ::vog;
  VOG_CHECK_ARG(step && (((uintptr_t)step) & 7) == 0);
  hipStream_t st = (hipStream_t)stream;
  if (phase == VOG_TICK_BEGIN) {
    if (!lens && n_lens == 0) return 0;                 // (a batch in a cached form carries no lengths: nothing to guard)
    VOG_CHECK_ARG(lens && n_lens > 0 && T > 0 && (((uintptr_t)lens) & 7) == 0);
    VOG_CHECK_ARG(capture ? (n_capture > 0 && (((uintptr_t)capture) & 7) == 0) : n_capture == 0);
    ::vog::launch(train_tick_begin_kernel, dim3(1), dim3(TICK_THREADS), 0, st, step, (long long*)lens, n_lens, T, (long long*)capture,
                  n_capture);
    VOG_LAUNCH_CHECK();
    return 0;
  }
  if (phase != VOG_TICK_END) VOG_FAIL(-1, "vog_train_tick: phase = %d, VOG_TICK_BEGIN (0) or VOG_TICK_END (1)", phase);
  if (loss_log) {
    VOG_CHECK_ARG(loss_src && log_rows > 0 && n_loss > 0 && n_loss < 64);
    VOG_CHECK_ARG(((((uintptr_t)loss_src) | ((uintptr_t)loss_log)) & 3) == 0);
  }
  ::vog::launch(train_tick_end_kernel, dim3(1), dim3(64), 0, st, step, loss_src, loss_log, log_rows, n_loss, count_adam ? 1 : 0);
  VOG_LAUNCH_CHECK();
  return 0;
}
