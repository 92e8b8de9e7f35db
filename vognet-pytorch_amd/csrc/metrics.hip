// Grounding metrics of a batch of prediction records on the device: GroundEval_SEP / _TEMP / _SPAT.eval_one_sent_idx
// (vognet-pytorch_amd/eval_fn_corr.py, the restatement of the reference's code/eval_fn_corr.py:302-747) for B records in
// ONE launch. A latency / byte kernel: per query a few KB of record, a few hundred bytes of annotation table and a few
// hundred float operations.
//
// Mapping: one 64-lane wave per query, four queries per workgroup; no LDS, no atomics, no state between records. The wave
// walks the sentence's groundable arguments (at most 15) and, per argument, spreads the inner list of the rule over its
// lanes - the argument's annotated (box, frame) pairs for "some annotated box is hit", the frames of a foreign video's
// segment for TEMP's "first frame above the threshold", the frames of the record for SPAT - and settles "any" / "first in
// list order" / "highest score, first on ties" with ballots, find-first and one shuffle reduction. Everything that indexes the
// table is wave-uniform (scalar loads); the record is read with per-lane loads whose addresses come from one level of table
// loads, so an argument costs two dependent memory levels.
//
// Exactness: the IoU is box_iou_f32 operation for operation in float32 WITHOUT contraction (hipcc would fuse `w * h` into
// the following subtraction and `(a2-a0) * (a3-a1)` into the area sum: one rounding less flips `> 0.5` on boundary boxes) and
// with the correctly rounded division; the score is compared as a double against the double threshold (the pickle turns it
// into a Python float). All other rules are integer logic, so the result word equals the host path's counts.
#include "val_dev.h"

namespace vog {

namespace {

constexpr int kErrVerb = 1 << 16;    // idx_verbs[targ_cmp] != idx_sent           (host: assert in eval_ground_acc)
constexpr int kErrMask = 1 << 17;    // SPAT chose a video with cmp_msk != 1      (host: assert in GroundEval_SPAT.argument)
constexpr int kErrRange = 1 << 18;   // sentence row / video / frame out of range  (host: IndexError)
constexpr int kVidW = 720;           // the SPAT shift per video slot (eval_fn_corr.py: 720 * targ)

// np.minimum / np.maximum: a NaN operand is the result (fminf / fmaxf would drop it)
__device__ __forceinline__ float np_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float np_max(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ float iou_f32(float a0, float a1, float a2, float a3, float b0, float b1, float b2, float b3) {
#pragma clang fp contract(off)
  const float area_a = (a2 - a0) * (a3 - a1);
  const float area_b = (b2 - b0) * (b3 - b1);
  const float w = np_max(np_min(a2, b2) - np_max(a0, b0), 0.f);
  const float h = np_max(np_min(a3, b3) - np_max(a1, b1), 0.f);
  const float inter = w * h;
  const float uni = (area_a + area_b) - inter;
  return __fdiv_rn(inter, uni);                  // 0/0 -> NaN: not a hit
}

struct Rec {
  const float* boxes;      // [nsrl][ncmp][nfrm0][7]
  const float* scores;     // [nsrl][ncmp][nfrm0]
  const int64_t* pcmp;     // [nsrl][nfrm0]
};

// GroundEval_SEP._hit of the prediction at (arg, video, frame) against annotated box `g` of the table (x shifted by `shift`)
__device__ __forceinline__ bool hit(const Rec& r, int64_t o, const int32_t* g, int shift, double thresh) {
  const float* pb = r.boxes + o * 7;
  const float v = iou_f32(pb[0], pb[1], pb[2], pb[3], (float)(g[0] + shift), (float)g[1], (float)(g[2] + shift), (float)g[3]);
  return v > 0.5f && (double)r.scores[o] > thresh;
}

}  // namespace

// `row`: NULL, or this launch's row of the result-word log (vog_gmetric_args.log): every word goes there as well
__device__ __forceinline__ void put_word(const vog_gmetric_args& a, int32_t* row, int q, int word) {
  a.result[q] = word;
  if (row) row[q] = word;
}

__device__ __forceinline__ void ground_metrics_body(const vog_gmetric_args& a, const vog_gmetric_table& t, int64_t rec_bytes, int32_t* row) {
  const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (q >= a.B) return;
  const int lane = threadIdx.x & 63;
  const int ncmp = a.ncmp, nfrm = a.nfrm0;
  const unsigned char* base = reinterpret_cast<const unsigned char*>(a.rec) + (int64_t)q * rec_bytes;
  const int64_t nb = (int64_t)a.nsrl * ncmp * nfrm;
  Rec r;
  r.boxes = reinterpret_cast<const float*>(base);
  r.scores = r.boxes + nb * 7;
  r.pcmp = reinterpret_cast<const int64_t*>(base + nb * 32);

  // ---- the query's metadata: lane v holds video v ---------------------------------------------------------------------
  const int64_t s64 = a.idx_sent[q], targ64 = a.targ_cmp[q];
  int64_t verb = 0, mskv = 0;
  if (lane < ncmp) {
    verb = a.idx_verbs[(int64_t)q * ncmp + lane];
    mskv = a.cmp_msk[(int64_t)q * ncmp + lane];
  }
  const unsigned long long bad_verb = __ballot(lane < ncmp && (verb < 0 || verb >= t.n_sent));
  const unsigned long long msk = __ballot(lane < ncmp && mskv == 1);
  int err = 0;
  if (bad_verb != 0 || s64 < 0 || s64 >= t.n_sent || targ64 < 0 || targ64 >= ncmp) err |= kErrRange;
  if (err) {                                       // nothing below may index with these values
    if (lane == 0) put_word(a, row, q, err);
    return;
  }
  const int s = (int)s64, targ = (int)targ64;
  if (a.idx_verbs[(int64_t)q * ncmp + targ] != s64) err |= kErrVerb;
  const int tot = t.n_ground[s];
  const int ao = t.arg_off[s], bo = t.box_off[s];
  int npred = t.arg_cnt[s];
  npred = npred < a.nsrl ? npred : a.nsrl;         // arguments past nsrl count in `tot` only (host: tot += 1, then a >= npred)
  if (tot == 0 || err) {                           // not scored (the host path returns None)
    if (lane == 0) put_word(a, row, q, err);
    return;
  }

  // ---- SEP: the video of the whole query = first-seen most frequent entry of pred_cmp -----------------------------------
  int query_vid = 0;
  if (a.conc_type == VOG_CONC_SEP) {
    const int n = a.nsrl * nfrm;
    int best_n = -1, best_first = 0x7fffffff;
    unsigned long long outside = 0;
    for (int c = 0; c < ncmp; ++c) {
      int cnt = 0, first = 0x7fffffff;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int64_t v = i < n ? r.pcmp[i] : -1;
        const unsigned long long m = __ballot(i < n && v == c);
        if (c == 0) outside |= __ballot(i < n && (v < 0 || v >= ncmp));
        cnt += __popcll(m);
        if (m != 0 && first == 0x7fffffff) first = i0 + __ffsll((long long)m) - 1;
      }
      if (cnt > best_n || (cnt == best_n && first < best_first)) { best_n = cnt; best_first = first; query_vid = c; }
    }
    if (outside != 0) {                            // not a video index: nothing the prediction head writes
      if (lane == 0) put_word(a, row, q, kErrRange);
      return;
    }
  }

  // ---- the arguments ------------------------------------------------------------------------------------------------------
  int res = 0, ndec = 0, d0 = 0;
  bool all_eq = true, all_targ = true;
  for (int arg = 0; arg < npred; ++arg) {
    if (t.has_box[ao + arg] != 1) continue;
    const int io = t.ind_off[ao + arg], ic = t.ind_cnt[ao + arg];
    bool ok = false;
    int dec = 0;

    // some annotated (box, frame) of the argument is hit in video v: lanes = the argument's annotated boxes
    auto any_hit = [&](int v) -> bool {
      unsigned long long m = 0;
      for (int j0 = 0; j0 < ic; j0 += 64) {
        const int j = j0 + lane;
        bool h = false;
        if (j < ic) {
          const int bi = bo + t.ind[io + j];
          const int f = t.gt_frm[bi];
          h = hit(r, ((int64_t)arg * ncmp + v) * nfrm + f, t.gt_box + (int64_t)bi * 4, 0, a.prob_thresh);
        }
        m |= __ballot(h);
      }
      return m != 0;
    };

    if (a.conc_type == VOG_CONC_SEP) {
      dec = query_vid;
      ok = query_vid == targ && any_hit(query_vid);
    } else if (a.conc_type == VOG_CONC_TEMP) {
      bool all_ok = true, fired = false;
      float fired_sc = 0.f;
      int fired_v = -1;
      for (int v = 0; v < ncmp; ++v) {
        if (!((msk >> v) & 1)) continue;
        if (v == targ) {
          if (!any_hit(v)) all_ok = false;
          continue;
        }
        // the FIRST frame, in the order of the foreign sentence's segment, scored above the threshold: lanes = that list
        const int sv = (int)a.idx_verbs[(int64_t)q * ncmp + v];
        const int fo = t.box_off[sv], fc = t.box_cnt[sv];
        const float* ps = r.scores + ((int64_t)arg * ncmp + v) * nfrm;
        for (int j0 = 0; j0 < fc; j0 += 64) {
          const int j = j0 + lane;
          float sc = 0.f;
          bool above = false;
          if (j < fc) {
            sc = ps[t.gt_frm[fo + j]];
            above = (double)sc > a.prob_thresh;
          }
          const unsigned long long m = __ballot(above);
          if (m != 0) {
            const float first_sc = __shfl(sc, __ffsll((long long)m) - 1);
            all_ok = false;
            if (!fired || first_sc > fired_sc) { fired_sc = first_sc; fired_v = v; }      // highest score, first on ties
            fired = true;
            break;
          }
        }
      }
      ok = all_ok;
      dec = all_ok ? targ : fired_v;               // fired_v = -1: nothing fired
    } else {
      // SPAT: lanes = the frames of the record
      bool all_ok = true, have_free = false;
      float free_sc = 0.f;
      int free_f = 0;
      for (int f0 = 0; f0 < nfrm; f0 += 64) {
        const int f = f0 + lane;
        bool bad = false, is_free = false, oob = false, masked = false;
        float sc = 0.f;
        if (f < nfrm) {
          const int64_t v64 = r.pcmp[(int64_t)arg * nfrm + f];
          oob = v64 < 0 || v64 >= ncmp;
          const int v = oob ? 0 : (int)v64;
          masked = !((msk >> v) & 1);
          const int64_t o = ((int64_t)arg * ncmp + v) * nfrm + f;
          sc = r.scores[o];
          bool annotated = false, h = false;
          for (int j = 0; j < ic; ++j) {           // (uniform trip count and table addresses; the predicate is per lane)
            const int bi = bo + t.ind[io + j];
            if (t.gt_frm[bi] != f) continue;
            annotated = true;
            if (v == targ && hit(r, o, t.gt_box + (int64_t)bi * 4, kVidW * targ, a.prob_thresh)) h = true;
          }
          if (annotated) {
            bad = !(v == targ && h);
          } else {
            bad = v != targ && (double)sc > a.prob_thresh;
            is_free = true;
          }
        }
        if (__ballot(oob) != 0) err |= kErrRange;
        else if (__ballot(masked) != 0) err |= kErrMask;
        if (__ballot(bad) != 0) all_ok = false;
        // the highest-scored free frame of this chunk, the first one on ties: (score, frame) reduction over the lanes
        const unsigned long long fm = __ballot(is_free);
        if (fm != 0) {
          float bs = is_free ? sc : 0.f;
          int bf = is_free ? f : 0x7fffffff;
          bool bv = is_free;
          for (int d = 32; d >= 1; d >>= 1) {
            const float os = __shfl_xor(bs, d);
            const int of = __shfl_xor(bf, d);
            const bool ov = __shfl_xor((int)bv, d) != 0;
            if (ov && (!bv || os > bs || (os == bs && of < bf))) { bs = os; bf = of; bv = true; }
          }
          if (!have_free || bs > free_sc) { free_sc = bs; free_f = bf; }
          have_free = true;
        }
      }
      ok = all_ok;
      dec = all_ok ? targ : (have_free ? -free_f : -5);       // frame 0 gives decision 0: the reference's quirk, kept
    }
    if (err) break;
    res += ok ? 1 : 0;
    if (ndec == 0) d0 = dec;
    all_eq = all_eq && dec == d0;
    all_targ = all_targ && dec == targ;
    ++ndec;
  }

  // ---- consistency / video accuracy of the per-argument decisions -------------------------------------------------------
  // (`all(d == most_common)` holds exactly when all decisions are equal, so the most common one never has to be counted)
  int cons = 0, vidf = 0;
  if (ndec > 0) {
    if (a.conc_type == VOG_CONC_SEP) { cons = 1; vidf = d0 == targ; }
    else if (a.conc_type == VOG_CONC_TEMP) { cons = all_eq && d0 >= 0; vidf = cons && d0 == targ; }
    else { cons = all_eq; vidf = all_targ; }
  }
  int word = err;
  if (!err) word = (res & 15) | ((tot & 15) << 4) | (cons << 8) | (vidf << 9) | ((res == tot ? 1 : 0) << 10);
  if (lane == 0) put_word(a, row, q, word);
}

__global__ __launch_bounds__(256) void ground_metrics_kernel(vog_gmetric_args a, vog_gmetric_table t, int64_t rec_bytes) {
  ground_metrics_body(a, t, rec_bytes, nullptr);
}

// The same with the validation log folded in (vog_gmetric_args.log): blocks [0, n_metric) score the records and write their
// words into row *lg.step of the word log as well; the blocks behind them copy the step's loss floats and records into their
// rows and set the marker (val_dev.h) - what vog_val_log would do in a launch of its own behind this one. Every block reads
// the step word itself; a step outside [0, rows) writes no row (the slot's own result words are still written).
__global__ __launch_bounds__(256) void ground_metrics_log_kernel(vog_gmetric_args a, vog_gmetric_table t, int64_t rec_bytes,
                                                                 vog_val_log_args lg, int n_metric) {
  const bool copy = (int)blockIdx.x >= n_metric;
  const int64_t tid = copy ? (int64_t)(blockIdx.x - n_metric) * 256 + threadIdx.x : 1;
  const int64_t s = val_log_row(lg, tid);
  if (copy) {
    if (s >= 0) val_log_copy(lg, s, tid, (int64_t)(gridDim.x - n_metric) * 256, false);
    return;
  }
  ground_metrics_body(a, t, rec_bytes, (s >= 0 && lg.word_log) ? lg.word_log + s * lg.B : nullptr);
}

// test entry: out[i] = box_iou_f32(a[i], b[i]) with the arithmetic of the metric kernel
__global__ __launch_bounds__(256) void box_iou_kernel(const float* a, const float* b, float* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* pa = a + (int64_t)i * 4;
  const float* pb = b + (int64_t)i * 4;
  out[i] = iou_f32(pa[0], pa[1], pa[2], pa[3], pb[0], pb[1], pb[2], pb[3]);
}

}  // namespace vog

extern "C" int vog_ground_metrics(const vog_gmetric_args* a, void* stream) {
  using namespace vog;
  VOG_CHECK_ARG(a && a->tab);
  VOG_CHECK_ARG(a->B >= 0 && a->ncmp > 0 && a->ncmp <= 64 && a->nsrl > 0 && a->nfrm0 > 0);
  VOG_CHECK_ARG(a->conc_type == VOG_CONC_SEP || a->conc_type == VOG_CONC_TEMP || a->conc_type == VOG_CONC_SPAT);
  if (a->B == 0) return 0;
  const vog_gmetric_table& t = *a->tab;
  VOG_CHECK_ARG(a->rec && a->idx_sent && a->idx_verbs && a->cmp_msk && a->targ_cmp && a->result);
  VOG_CHECK_ARG(t.n_sent > 0 && t.box_off && t.box_cnt && t.arg_off && t.arg_cnt && t.n_ground);
  VOG_CHECK_ARG(t.n_box == 0 || (t.gt_box && t.gt_frm));
  VOG_CHECK_ARG(t.n_arg == 0 || (t.has_box && t.ind_off && t.ind_cnt));
  VOG_CHECK_ARG(t.n_ind == 0 || t.ind);
  if (t.nfrm0 != a->nfrm0)
    VOG_FAIL(-1, "vog_ground_metrics: the annotation table was checked for %d frames, the records hold %d", t.nfrm0, a->nfrm0);
  const int64_t rec_bytes = vog_pred_record_bytes(a->ncmp, a->nsrl, a->nfrm0);
  const int n_metric = (a->B + 3) / 4;
  if (a->log) {
    VOG_TRY(val_log_check(a->log));
    VOG_CHECK_ARG(a->log->B == a->B);
    ::vog::launch(ground_metrics_log_kernel, dim3((unsigned)(n_metric + val_log_blocks(*a->log))), dim3(256), 0, (hipStream_t)stream,
                  *a, t, rec_bytes, *a->log, n_metric);
    VOG_LAUNCH_CHECK();
    return 0;
  }
  ::vog::launch(ground_metrics_kernel, dim3((unsigned)n_metric), dim3(256), 0, (hipStream_t)stream, *a, t, rec_bytes);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_box_iou_f32(const float* a, const float* b, float* out, int n, void* stream) {
  using namespace vog;
  VOG_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  VOG_CHECK_ARG(a && b && out);
  ::vog::launch(box_iou_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  VOG_LAUNCH_CHECK();
  return 0;
}
