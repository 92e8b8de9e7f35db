// Device side of the validation log (vog_val_log, csrc/val.hip), shared with the metrics kernel that writes its row of the
// logs itself (vog_gmetric_args.log, csrc/metrics.hip).
#pragma once
#include "common.h"

namespace vog {

// n 4-byte words src -> dst by the threads [tid, tid + nthr, ...) of the launch: 16 bytes per lane wherever source and
// destination share their 16-byte phase, single words in front of and behind that body
__device__ __forceinline__ void copy_words(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t n, int64_t tid,
                                           int64_t nthr) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
  if (((sa ^ da) & 15) != 0) {                       // no common 16-byte phase: single words throughout
    for (int64_t i = tid; i < n; i += nthr) dst[i] = src[i];
    return;
  }
  int64_t head = (int64_t)(((16 - (da & 15)) & 15) >> 2);      // words in front of the first 16-byte boundary
  head = head < n ? head : n;
  const int64_t n4 = (n - head) >> 2;
  for (int64_t i = tid; i < head; i += nthr) dst[i] = src[i];
  const u32x4* s4 = reinterpret_cast<const u32x4*>(src + head);
  u32x4* d4 = reinterpret_cast<u32x4*>(dst + head);
  for (int64_t i = tid; i < n4; i += nthr) d4[i] = s4[i];
  for (int64_t i = head + (n4 << 2) + tid; i < n; i += nthr) dst[i] = src[i];
}

// the row of this launch, or -1 (nothing may index with it; thread `tid` 0 reports it)
__device__ __forceinline__ int64_t val_log_row(const vog_val_log_args& a, int64_t tid) {
  const int64_t s = *a.step;
  if (s >= 0 && s < a.rows) return s;
  if (tid == 0 && a.bad_step) *a.bad_step = 1u;
  return -1;
}

// the copies of one step into row s (s valid) by threads [tid, tid + nthr, ...); `words`: also the result words
__device__ __forceinline__ void val_log_copy(const vog_val_log_args& a, int64_t s, int64_t tid, int64_t nthr, bool words) {
  if (a.loss_src) copy_words(reinterpret_cast<const uint32_t*>(a.loss_src), reinterpret_cast<uint32_t*>(a.loss_log + s * 6), 6, tid, nthr);
  if (words && a.word_src)
    copy_words(reinterpret_cast<const uint32_t*>(a.word_src), reinterpret_cast<uint32_t*>(a.word_log + s * a.B), a.B, tid, nthr);
  if (a.rec_src) {
    const int64_t n = (int64_t)a.B * a.rec_words;
    copy_words(reinterpret_cast<const uint32_t*>(a.rec_src), reinterpret_cast<uint32_t*>(a.rec_log + s * n), n, tid, nthr);
  }
  if (tid == 0 && a.written) a.written[s] = 1;
}

// host checks of a log argument block, shared by vog_val_log and vog_ground_metrics (defined in val.hip)
int val_log_check(const vog_val_log_args* a);

// blocks of 256 threads for the copies of one step
inline int64_t val_log_blocks(const vog_val_log_args& a) {
  const int64_t words = 6 + (int64_t)a.B + (a.rec_src ? (int64_t)a.B * a.rec_words : 0);
  const int64_t gx = (words + 1023) / 1024;          // one 16-byte chunk per lane ...
  return gx < 1 ? 1 : (gx > 256 ? 256 : gx);         // ... up to one block per CU
}

}  // namespace vog
