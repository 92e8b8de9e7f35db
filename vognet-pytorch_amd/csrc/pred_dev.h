// Per-frame arg-max + box gather of the prediction head (Evaluator*.get_out_results_boxes,
// code/eval_vsrl_corr.py:162-424) as a device function of the work-item index: the stand-alone kernel
// (elementwise.hip) and the tail of the last mul_tx encoder-layer tail (txtail_dev.h: the workgroup that
// finishes last runs the head for the whole batch) share it, so both forms are bit-identical.
#pragma once
#include "common.h"

namespace vog {

// COHERENT: outs_eval was written by other workgroups of the SAME launch (write-through stores): L1/L2-bypassing loads
template <bool COHERENT>
__device__ __forceinline__ float pred_ld(const float* base, int64_t i) {
  if (!COHERENT) return base[i];
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0x7fffffff, 0x00020000);
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4), 0, 16 /* sc1 */));
}

constexpr int PRED_NP = 8, PRED_NC = 4;      // the one-round form of pred_item: proposals per frame, videos per query
static_assert(PRED_NC == 4, "pred_item selects the other videos' maxima by hand");

template <bool COHERENT>
__device__ __forceinline__ void pred_item(const vog_pred_args& a, int64_t rec_bytes, int i) {

  // one thread per (query, arg, frame, video): arg-max over the proposals of that video's frame
  // and the box gather; the thread of video 0 also does the pred_cmp arg-max over the videos
  // (it re-reads the ncmp x nppf0 scores: all addresses are known up front, so the kernel is two
  // dependent memory levels deep instead of 2 x ncmp)
  const int per_q = a.nsrl * a.nfrm0 * a.ncmp;
  if (i >= a.B * per_q) return;
  const int b = i / per_q, r = i % per_q;
  const int arg = r / (a.nfrm0 * a.ncmp), f = (r / a.ncmp) % a.nfrm0, c = r % a.ncmp;
  const int npv = a.nfrm0 * a.nppf0;
  unsigned char* rec = reinterpret_cast<unsigned char*>(a.rec) + (int64_t)b * rec_bytes;
  float* boxes = reinterpret_cast<float*>(rec);
  float* scores = boxes + (int64_t)a.nsrl * a.ncmp * a.nfrm0 * 7;
  int64_t* idx = reinterpret_cast<int64_t*>(rec + (int64_t)a.nsrl * a.ncmp * a.nfrm0 * 8 * 4);
  auto first_prop = [&](int cc, int64_t* e0, int64_t* p0) {   // in outs_eval / in props
    if (a.conc_type == VOG_CONC_SPAT) {
      const int r0 = (f * a.ncmp + cc) * a.nppf0;
      *e0 = ((int64_t)b * a.nsrl + arg) * ((int64_t)a.ncmp * npv) + r0;
      *p0 = (int64_t)b * a.ncmp * npv + r0;
    } else if (a.conc_type == VOG_CONC_TEMP) {
      const int r0 = (cc * a.nfrm0 + f) * a.nppf0;
      *e0 = ((int64_t)b * a.nsrl + arg) * ((int64_t)a.ncmp * npv) + r0;
      *p0 = (int64_t)b * a.ncmp * npv + r0;
    } else {
      *e0 = (((int64_t)b * a.ncmp + cc) * a.nsrl + arg) * npv + (int64_t)f * a.nppf0;
      *p0 = ((int64_t)b * a.ncmp + cc) * npv + (int64_t)f * a.nppf0;
    }
  };
  int64_t e0, p0;
  first_prop(c, &e0, &p0);
  const int64_t o = ((int64_t)arg * a.ncmp + c) * a.nfrm0 + f;
  // Few proposals per frame (gt5: 5) and few videos: the frame's scores, ALL its candidate boxes and (video 0's thread) the
  // other videos' scores are requested together, so the box gather behind the arg-max is a register select and not a second
  // trip to memory. Same comparisons in the same order as the general form: same records.
  const bool few = a.nppf0 >= 1 && a.nppf0 <= PRED_NP && a.ncmp <= PRED_NC;
  const bool cross = c == 0 && a.conc_type == VOG_CONC_SPAT;
  float best, box[7], best_o[PRED_NC - 1];       // best_o: the frame's maximum in videos 1 .. ncmp - 1 (few && cross)
  if (few) {
    // (clamped indices, not guards: a guarded load is a branch, and the compiler waits for memory at the end of every one)
    float sc[PRED_NP], bx[PRED_NP][7], oth[PRED_NC - 1][PRED_NP];
    const int kl = a.nppf0 - 1;
#pragma unroll
    for (int k = 0; k < PRED_NP; ++k) sc[k] = pred_ld<COHERENT>(a.outs_eval, e0 + (k < kl ? k : kl));
#pragma unroll
    for (int k = 0; k < PRED_NP; ++k) {
      const float* pr = a.props + (p0 + (k < kl ? k : kl)) * 7;
#pragma unroll
      for (int j = 0; j < 7; ++j) bx[k][j] = pr[j];
    }
#pragma unroll
    for (int cc = 1; cc < PRED_NC; ++cc)
#pragma unroll
      for (int k = 0; k < PRED_NP; ++k) oth[cc - 1][k] = 0.f;
    if (cross) {
#pragma unroll
      for (int cc = 1; cc < PRED_NC; ++cc) {
        int64_t e1, p1;
        first_prop(cc < a.ncmp ? cc : a.ncmp - 1, &e1, &p1);
#pragma unroll
        for (int k = 0; k < PRED_NP; ++k) oth[cc - 1][k] = pred_ld<COHERENT>(a.outs_eval, e1 + (k < kl ? k : kl));
      }
    }
    best = sc[0];
    int bi = 0;
#pragma unroll
    for (int k = 1; k < PRED_NP; ++k)
      if (k < a.nppf0 && sc[k] > best) { best = sc[k]; bi = k; }          // first maximum wins (torch.max on CPU)
#pragma unroll
    for (int j = 0; j < 7; ++j) box[j] = bx[0][j];
#pragma unroll
    for (int k = 1; k < PRED_NP; ++k)
#pragma unroll
      for (int j = 0; j < 7; ++j) box[j] = k == bi ? bx[k][j] : box[j];
#pragma unroll
    for (int cc = 1; cc < PRED_NC; ++cc) {
      float bc = oth[cc - 1][0];
#pragma unroll
      for (int k = 1; k < PRED_NP; ++k)
        if (k < a.nppf0) bc = fmaxf(bc, oth[cc - 1][k]);
      best_o[cc - 1] = bc;
    }
  } else {
    best = pred_ld<COHERENT>(a.outs_eval, e0);
    int bi = 0;
    for (int k = 1; k < a.nppf0; ++k) {
      const float v = pred_ld<COHERENT>(a.outs_eval, e0 + k);
      if (v > best) { best = v; bi = k; }          // first maximum wins (torch.max on CPU)
    }
    const float* pr = a.props + (p0 + bi) * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) box[k] = pr[k];
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) boxes[o * 7 + k] = box[k];
  scores[o] = best;
  if (c != 0) return;
  int64_t out = 0;
  if (a.conc_type == VOG_CONC_SPAT) {
    float best_c = best;                         // video 0; first maximum over the videos
    for (int cc = 1; cc < a.ncmp; ++cc) {
      float bc;
      if (few) {
        bc = cc == 1 ? best_o[0] : (cc == 2 ? best_o[1] : best_o[2]);
      } else {
        int64_t e1, p1;
        first_prop(cc, &e1, &p1);
        bc = pred_ld<COHERENT>(a.outs_eval, e1);
        for (int k = 1; k < a.nppf0; ++k) bc = fmaxf(bc, pred_ld<COHERENT>(a.outs_eval, e1 + k));
      }
      if (bc > best_c) { best_c = bc; out = cc; }
    }
  } else if (a.conc_type == VOG_CONC_SEP) {
    float bf = a.fin_scores[(int64_t)b * a.ncmp];
    for (int cc = 1; cc < a.ncmp; ++cc) {
      const float v = a.fin_scores[(int64_t)b * a.ncmp + cc];
      if (v > bf) { bf = v; out = cc; }
    }
  }
  idx[(int64_t)arg * a.nfrm0 + f] = out;
}

}  // namespace vog
