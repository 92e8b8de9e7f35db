// Validation log: one step's results -> row `step` of caller-owned device logs (vog_val_log, include/vog_hip.h).
//
// A validation step ends with three small results at FIXED addresses - the 6 floats of vog_loss_fwd, the B result words of
// vog_ground_metrics, the B prediction records - and a captured graph can only ever write to fixed addresses. The row a
// launch writes is therefore chosen on the device: `step` is a word in device memory whose CONTENTS change per launch (a fed
// graph copies it from the staging buffer with the rest of the batch). The host reads the logs once, behind the loop.
//
// A byte kernel: 27 KB of records per small batch, 6.8 KB per query at cfg 2. The three copies share one launch: every block
// strides over the words of all three, 16 bytes per lane wherever source and destination share their alignment (the row offset
// step * B * rec_words is not a multiple of 4 words for every record width), single words in front of and behind that body.
// Each launch writes its own row only: no atomics, no state between launches. A step outside [0, rows) forms no address.
// Inside a fed graph with device metrics the copies ride in the metrics launch instead (vog_gmetric_args.log, csrc/metrics.hip:
// its waves write their result words into the row themselves, extra blocks copy loss and records); this stand-alone form
// serves the short tail batch and validation without device metrics. The device code of both is csrc/val_dev.h.
#include "val_dev.h"

namespace vog {

__global__ __launch_bounds__(256) void val_log_kernel(vog_val_log_args a) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
  const int64_t s = val_log_row(a, tid);
  if (s < 0) return;                                 // (uniform)
  val_log_copy(a, s, tid, nthr, true);
}

int val_log_check(const vog_val_log_args* a) {
  VOG_CHECK_ARG(a && a->step && a->rows > 0 && a->B >= 0 && a->rec_words >= 0);
  VOG_CHECK_ARG((a->loss_src == nullptr) == (a->loss_log == nullptr));
  VOG_CHECK_ARG((a->rec_src == nullptr) == (a->rec_log == nullptr));
  VOG_CHECK_ARG(!a->rec_src || a->rec_words > 0);
  VOG_CHECK_ARG((((uintptr_t)a->loss_src | (uintptr_t)a->loss_log | (uintptr_t)a->word_src | (uintptr_t)a->word_log |
                  (uintptr_t)a->rec_src | (uintptr_t)a->rec_log | (uintptr_t)a->step | (uintptr_t)a->written |
                  (uintptr_t)a->bad_step) & 3) == 0);
  return 0;
}

}  // namespace vog

extern "C" int vog_val_log(const vog_val_log_args* a, void* stream) {
  using namespace vog;
  VOG_TRY(val_log_check(a));
  VOG_CHECK_ARG((a->word_src == nullptr) == (a->word_log == nullptr));
  ::vog::launch(val_log_kernel, dim3((unsigned)val_log_blocks(*a)), dim3(256), 0, (hipStream_t)stream, *a);
  VOG_LAUNCH_CHECK();
  return 0;
}
