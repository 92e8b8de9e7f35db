// Device-side SPAT / TEMP batch assembly: verb_item_getter_SPAT / _TEMP
// (code/dat_loader_simple.py:1046-1338) for a whole batch of queries, writing straight into the
// forward's / loss's input buffers. Pure layout work on the 2 MB/query feature block:
//   SPAT: proposals x1, x2 += 720 * video, rows re-ordered (video, frame, prop) -> (frame, video, prop);
//         region features and the proposal padding mask re-ordered the same way; per-frame segment
//         features (video, frame) -> (frame, video)
//   TEMP: proposal frame index += 10 * video; everything else is the plain concatenation
//   both: ground-truth boxes shifted the same way, the first num_box[v] of every video concatenated
//         and zero padded (the reference's gt[0, 0] fallback when there are none); srl_boxes shifted
//         by the boxes in front of the target video where srl_boxes_lens > 0; frm_mask[r, g] =
//         (frame(proposal r) != frame(gt g)) for g < total boxes, else 1.
// HBM bound: every byte is read once and written once with 16-byte accesses (feature rows) by
// `assemble_rows_kernel`; `assemble_gt_kernel` (one workgroup per query) does the KB-sized part.
// Bit-exact vs the reference (fp32 adds of small integers * 720 / * 10, otherwise copies).
// Also here: the same assembly from a feature bank (`bank_*_kernel`), `copy_segments_kernel`, and the query bank's
// `gather_rows_kernel` (rows of up to 32 small tables through one index, one launch).
#include "common.h"

namespace vog {

__global__ __launch_bounds__(256) void assemble_rows_kernel(vog_assemble_args a) {
  const int NPv = a.nfrm0 * a.nppf0;
  const int64_t n_prop_rows = (int64_t)a.B * a.ncmp * NPv;
  const int64_t n_seg_rows = (int64_t)a.B * a.ncmp * a.nfrm0;
  const int64_t row = blockIdx.x;
  const bool spat = a.conc_type == VOG_CONC_SPAT;
  if (row < n_prop_rows) {
    // source row (b, v, f, p)
    const int b = (int)(row / ((int64_t)a.ncmp * NPv));
    int r = (int)(row - (int64_t)b * a.ncmp * NPv);
    const int v = r / NPv; r -= v * NPv;
    const int f = r / a.nppf0, p = r - f * a.nppf0;
    const int64_t dst = (int64_t)b * a.ncmp * NPv +
                        (spat ? ((int64_t)f * a.ncmp + v) * a.nppf0 + p : (int64_t)v * NPv + f * a.nppf0 + p);
    const float4* s4 = reinterpret_cast<const float4*>(a.region_in + row * a.prop_dim);
    float4* d4 = reinterpret_cast<float4*>(a.region_out + dst * a.prop_dim);
    for (int i = threadIdx.x; i < a.prop_dim / 4; i += 256) d4[i] = s4[i];
    if (threadIdx.x < 7) {
      float x = a.props_in[row * 7 + threadIdx.x];
      const int c = threadIdx.x;
      if (spat && (c == 0 || c == 2)) x = x + (float)v * a.vid_w;
      if (!spat && c == 4) x = x + (float)v * (float)a.nfrm0;
      a.props_out[dst * 7 + c] = x;
    }
    if (threadIdx.x == 7 && a.pnt_in) a.pnt_out[dst] = a.pnt_in[row];
    return;
  }
  const int64_t srow = row - n_prop_rows;
  if (srow >= n_seg_rows) return;
  const int b = (int)(srow / ((int64_t)a.ncmp * a.nfrm0));
  const int r = (int)(srow - (int64_t)b * a.ncmp * a.nfrm0);
  const int v = r / a.nfrm0, f = r - v * a.nfrm0;
  const int64_t dst = (int64_t)b * a.ncmp * a.nfrm0 + (spat ? (int64_t)f * a.ncmp + v : (int64_t)r);
  const float4* s4 = reinterpret_cast<const float4*>(a.seg_in + srow * a.seg_dim);
  float4* d4 = reinterpret_cast<float4*>(a.seg_out + dst * a.seg_dim);
  for (int i = threadIdx.x; i < a.seg_dim / 4; i += 256) d4[i] = s4[i];
}

// Where the per-video loss-side items of query b come from: `row(b, v)` names video v's row of the gt / num_box tables
// (-1: none, the video counts as one without boxes).
struct ItemSrc {                       // per-video items of the batch itself, [B, ncmp, ...]
  const float* gt; const int64_t* num_box; int ncmp;
  __device__ int64_t row(int b, int v) const { return (int64_t)b * ncmp + v; }
};
struct BankSrc {                       // rows of a feature bank through index [B, ncmp]; an index outside [0, V) forms no address
  const float* gt; const int64_t* num_box; const int32_t* index; int64_t V; int ncmp;
  __device__ int64_t row(int b, int v) const {
    const int64_t i = index[(int64_t)b * ncmp + v];
    return (i >= 0 && i < V) ? i : -1;
  }
};

// one workgroup per query: gt boxes, srl_boxes, frame mask (reads props_out of THIS query: launched after
// the rows kernel on the same stream). A = vog_assemble_args | vog_bank_assemble_args (same output members).
template <typename A, typename Src>
__device__ __forceinline__ void assemble_gt_body(const A& a, const Src& src) {
  __shared__ int cum[65];
  __shared__ int64_t vrow[64];
  __shared__ float gfrm[1024];
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool spat = a.conc_type == VOG_CONC_SPAT;
  const int NPt = a.ncmp * a.nfrm0 * a.nppf0;
  if (tid < a.ncmp) vrow[tid] = src.row(b, tid);
  __syncthreads();
  if (tid == 0) {
    cum[0] = 0;
    for (int v = 0; v < a.ncmp; ++v) cum[v + 1] = cum[v] + (vrow[v] >= 0 ? (int)src.num_box[vrow[v]] : 0);
  }
  __syncthreads();
  const int total = cum[a.ncmp];
  const int n_rows = total > 0 ? total : 1;                 // the reference's gt[0, 0] fallback
  float* gout = a.gt_out + (int64_t)b * a.G * 5;
  for (int i = tid; i < a.G * 5; i += 256) {
    const int g = i / 5, c = i - g * 5;
    float x = 0.f;
    if (g < n_rows && g < a.G) {
      int v = 0, k = 0;
      if (total > 0) { while (g >= cum[v + 1]) ++v; k = g - cum[v]; }
      if (vrow[v] >= 0) {
        x = src.gt[(vrow[v] * a.G + k) * 5 + c];
        if (spat && (c == 0 || c == 2)) x = x + (float)v * a.vid_w;
        if (!spat && c == 4) x = x + (float)v * (float)a.nfrm0;
      }
    }
    gout[i] = x;
    if (c == 4 && g < 1024) gfrm[g] = x;
  }
  if (tid == 0) a.num_box_out[b] = total;
  const int shift = cum[(int)a.target_cmp[b]];
  const int nsb = a.nv * a.nsrl * a.nbox;
  for (int i = tid; i < nsb; i += 256) {
    const int64_t j = (int64_t)b * nsb + i;
    a.srl_boxes_out[j] = a.srl_boxes_in[j] + (a.srl_boxes_lens[j] > 0 ? shift : 0);
  }
  __syncthreads();
  unsigned char* fm = a.frm_out + (int64_t)b * NPt * a.G;
  const float* pout = a.props_out + (int64_t)b * NPt * 7;
  for (int i = tid; i < NPt * a.G; i += 256) {
    const int r = i / a.G, g = i - r * a.G;
    fm[i] = g < total ? (unsigned char)(pout[(int64_t)r * 7 + 4] != gfrm[g]) : (unsigned char)1;
  }
}

__global__ __launch_bounds__(256) void assemble_gt_kernel(vog_assemble_args a) {
  assemble_gt_body(a, ItemSrc{a.gt_in, a.num_box, a.ncmp});
}

// ---- feature bank: the same assembly, every per-video row read through index [B, ncmp] ------------------------------
// One 256-thread workgroup per destination row (the shape of assemble_rows_kernel); the row's video index is wave-uniform
// and read once. A region row is 4096 B (f16) / 8192 B (fp32), a seg row 6144 / 12288 B: 16-byte loads, eight halves
// become two float4 stores (f16 -> fp32 is exact). A row whose index lies outside [0, V) is written as zeros.
template <typename T> struct BankRow;
template <> struct BankRow<float> {
  static __device__ __forceinline__ void gather(const void* tab, int64_t src_row, float* dst, int dim, bool ok) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(tab) + (ok ? src_row * (dim / 4) : 0);
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
    for (int i = threadIdx.x; i < dim / 4; i += 256) d4[i] = ok ? s4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
};
template <> struct BankRow<_Float16> {
  static __device__ __forceinline__ void gather(const void* tab, int64_t src_row, float* dst, int dim, bool ok) {
    const f16x8_t* s8 = reinterpret_cast<const f16x8_t*>(tab) + (ok ? src_row * (dim / 8) : 0);
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
    for (int i = threadIdx.x; i < dim / 8; i += 256) {
      f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
      if (ok) {
        const f16x8_t h = s8[i];
        lo = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        hi = f32x4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
      }
      d4[2 * i] = lo;
      d4[2 * i + 1] = hi;
    }
  }
};

template <typename T>
__global__ __launch_bounds__(256) void bank_rows_kernel(vog_bank_assemble_args a) {
  const int NPv = a.nfrm0 * a.nppf0;
  const int64_t n_prop_rows = (int64_t)a.B * a.ncmp * NPv;
  const int64_t n_seg_rows = (int64_t)a.B * a.ncmp * a.nfrm0;
  const int64_t row = blockIdx.x;
  const bool spat = a.conc_type == VOG_CONC_SPAT, temp = a.conc_type == VOG_CONC_TEMP;
  if (row < n_prop_rows) {
    // (b, v, f, p) of the gathered [B, ncmp, NPv] order
    const int b = (int)(row / ((int64_t)a.ncmp * NPv));
    int r = (int)(row - (int64_t)b * a.ncmp * NPv);
    const int v = r / NPv; r -= v * NPv;
    const int f = r / a.nppf0, p = r - f * a.nppf0;
    const int64_t vid = a.index[(int64_t)b * a.ncmp + v];
    const bool ok = vid >= 0 && vid < a.bank.V;
    const int64_t src = ok ? vid * NPv + r : 0;
    const int64_t dst = spat ? (int64_t)b * a.ncmp * NPv + ((int64_t)f * a.ncmp + v) * a.nppf0 + p : row;
    BankRow<T>::gather(a.bank.region, src, a.region_out + dst * a.prop_dim, a.prop_dim, ok);
    if (threadIdx.x < 7) {
      const int c = threadIdx.x;
      float x = 0.f;
      if (ok) {
        x = a.bank.props[src * 7 + c];
        if (spat && (c == 0 || c == 2)) x = x + (float)v * a.vid_w;
        if (temp && c == 4) x = x + (float)v * (float)a.nfrm0;
      }
      a.props_out[dst * 7 + c] = x;
    }
    if (threadIdx.x == 7 && a.pnt_out) a.pnt_out[dst] = ok ? a.bank.pnt[src] : (unsigned char)0;
    if (threadIdx.x == 8 && !ok && a.bad_index) *a.bad_index = 1u;
    return;
  }
  const int64_t srow = row - n_prop_rows;
  if (srow >= n_seg_rows) return;
  const int b = (int)(srow / ((int64_t)a.ncmp * a.nfrm0));
  const int r = (int)(srow - (int64_t)b * a.ncmp * a.nfrm0);
  const int v = r / a.nfrm0, f = r - v * a.nfrm0;
  const int64_t vid = a.index[(int64_t)b * a.ncmp + v];
  const bool ok = vid >= 0 && vid < a.bank.V;
  const int64_t dst = spat ? (int64_t)b * a.ncmp * a.nfrm0 + (int64_t)f * a.ncmp + v : srow;
  BankRow<T>::gather(a.bank.seg, ok ? vid * a.nfrm0 + f : 0, a.seg_out + dst * a.seg_dim, a.seg_dim, ok);
}

__global__ __launch_bounds__(256) void bank_gt_kernel(vog_bank_assemble_args a) {
  assemble_gt_body(a, BankSrc{a.bank.gt, a.bank.num_box, a.index, a.bank.V, a.ncmp});
}

// SEP: gt boxes and box counts of every (query, video) as they are; one workgroup per (b, v). frm_out (optional): the
// video's own frame mask [NPv, G] as the loader pads it (code/dat_loader_simple.py:405-416, get_frm_mask :237-255):
// frame(proposal r) != frame(gt g) for r < the video's real proposals and g < num_box, 1 everywhere else. The bank keeps no
// proposal count: the real proposals end behind the last nonzero byte of the video's pnt row (padding rows are zero there).
__global__ __launch_bounds__(256) void bank_gt_sep_kernel(vog_bank_assemble_args a) {
  __shared__ int n_real;
  const int64_t bv = blockIdx.x;
  const int64_t vid = a.index[bv];
  const bool ok = vid >= 0 && vid < a.bank.V;
  const float* g = a.bank.gt + (ok ? vid : 0) * a.G * 5;
  float* o = a.gt_out + bv * a.G * 5;
  for (int i = threadIdx.x; i < a.G * 5; i += 256) o[i] = ok ? g[i] : 0.f;
  const int64_t nb64 = ok ? a.bank.num_box[vid] : 0;
  if (threadIdx.x == 0) a.num_box_out[bv] = nb64;
  if (!a.frm_out) return;                              // (uniform)
  const int NPv = a.nfrm0 * a.nppf0;
  if (threadIdx.x == 0) n_real = 0;
  __syncthreads();
  if (ok) {
    const unsigned char* pm = a.bank.pnt + vid * NPv;
    int last = 0;
    for (int r = threadIdx.x; r < NPv; r += 256) last = pm[r] ? r + 1 : last;
    if (last > 0) atomicMax(&n_real, last);            // (LDS; the order does not matter for a maximum)
  }
  __syncthreads();
  const int np = n_real;
  const int nb = (int)(nb64 < 0 ? 0 : (nb64 > a.G ? a.G : nb64));
  const float* pr = a.bank.props + (ok ? vid : 0) * NPv * 7;
  unsigned char* fm = a.frm_out + bv * NPv * a.G;
  for (int i = threadIdx.x; i < NPv * a.G; i += 256) {
    const int r = i / a.G, c = i - r * a.G;
    fm[i] = (r < np && c < nb) ? (unsigned char)(pr[(int64_t)r * 7 + 4] != g[(int64_t)c * 5 + 4]) : (unsigned char)1;
  }
}

// byte ranges src -> dst, one launch: blockIdx.y = segment, the blocks of a segment stride over its 16-byte chunks.
// The sources may be PINNED HOST memory (mapped into the device's address space): the loads then cross the host link,
// which wants many 16-byte requests in flight and nothing else - no staging copy, no DMA set-up latency.
struct CopySegs { vog_copy_seg s[VOG_MAX_COPY_SEGS]; };
__global__ __launch_bounds__(256) void copy_segments_kernel(CopySegs cs) {
  const vog_copy_seg sg = cs.s[blockIdx.y];
  const size_t n16 = sg.bytes >> 4;
  const u32x4* s4 = reinterpret_cast<const u32x4*>(sg.src);
  u32x4* d4 = reinterpret_cast<u32x4*>(sg.dst);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) d4[i] = s4[i];
  if (blockIdx.x == 0) {
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(sg.src);
    unsigned char* db = reinterpret_cast<unsigned char*>(sg.dst);
    for (size_t i = (n16 << 4) + threadIdx.x; i < sg.bytes; i += 256) db[i] = sb[i];
  }
}

// ---- query bank: rows of several tables through ONE index, one launch -----------------------------------------------------------
// blockIdx.y = key; the blocks of a key stride over its units of `1 << lg` bytes (the widest of 16 / 8 / 4 / 1 that the
// table, the destination and the row length share; chosen on the host). A per-batch key is one plain range. A row number
// outside [0, Q) forms no address: its destination row is zeros and the sticky word is set. The key table travels in the
// kernel arguments (nothing is uploaded: the launch can be captured), 24 bytes per key.
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
struct GatherKey { const unsigned char* table; unsigned char* dst; int32_t row_bytes; int32_t mode; };   // mode = lg | per_batch << 8
struct GatherKeys {
  const int32_t* index; uint32_t* bad; int64_t Q; int32_t B, n_keys;
  GatherKey k[VOG_MAX_GATHER_KEYS];
};
static_assert(sizeof(GatherKeys) <= 1024, "the key table must fit a launch record's arguments");

template <typename V>
__device__ __forceinline__ void gather_key(const GatherKey& k, const GatherKeys& g, bool per_batch) {
  const int64_t upr = k.row_bytes / (int)sizeof(V);                  // units per row
  const int64_t n = per_batch ? upr : (int64_t)g.B * upr;
  const V* tab = reinterpret_cast<const V*>(k.table);
  V* dst = reinterpret_cast<V*>(k.dst);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    V v = V(0);
    if (per_batch) {
      v = tab[i];
    } else {
      const int64_t b = i / upr, u = i - b * upr;
      const int64_t r = g.index[b];
      if (r >= 0 && r < g.Q) v = tab[r * upr + u];
      else if (u == 0 && g.bad) *g.bad = 1u;
    }
    dst[i] = v;
  }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(GatherKeys g) {
  const GatherKey k = g.k[blockIdx.y];
  const bool per_batch = (k.mode >> 8) != 0;
  switch (k.mode & 255) {                                            // (uniform per block)
    case 4: gather_key<u32x4>(k, g, per_batch); break;
    case 3: gather_key<u32x2>(k, g, per_batch); break;
    case 2: gather_key<unsigned int>(k, g, per_batch); break;
    default: gather_key<unsigned char>(k, g, per_batch); break;
  }
}

}  // namespace vog

extern "C" int vog_gather_rows(const vog_gather_args* a, void* stream) {
  using namespace vog;
  VOG_CHECK_ARG(a && a->index && a->B > 0 && a->Q > 0 && a->Q <= 0x7fffffffLL);
  VOG_CHECK_ARG(a->n_keys >= 1 && a->n_keys <= VOG_MAX_GATHER_KEYS);
  GatherKeys g;
  memset(&g, 0, sizeof(g));
  g.index = a->index; g.bad = a->bad_index; g.Q = a->Q; g.B = a->B; g.n_keys = a->n_keys;
  int64_t mx = 0;
  for (int i = 0; i < a->n_keys; ++i) {
    const vog_gather_key& k = a->keys[i];
    VOG_CHECK_ARG(k.table && k.dst && k.row_bytes > 0 && k.row_bytes <= 0x7fffffffLL);
    const uintptr_t m = (uintptr_t)k.table | (uintptr_t)k.dst | (uintptr_t)k.row_bytes;
    const int lg = (m & 15) == 0 ? 4 : ((m & 7) == 0 ? 3 : ((m & 3) == 0 ? 2 : 0));
    g.k[i].table = reinterpret_cast<const unsigned char*>(k.table);
    g.k[i].dst = reinterpret_cast<unsigned char*>(k.dst);
    g.k[i].row_bytes = (int32_t)k.row_bytes;
    g.k[i].mode = lg | (k.per_batch ? 256 : 0);
    const int64_t units = (k.per_batch ? 1 : (int64_t)a->B) * (k.row_bytes >> lg);
    mx = units > mx ? units : mx;
  }
  int64_t gx = (mx + 255) / 256;                            // one unit per thread for the largest key, up to 256 blocks
  gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
  ::vog::launch(gather_rows_kernel, dim3((unsigned)gx, (unsigned)a->n_keys), dim3(256), 0, (hipStream_t)stream, g);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_copy_segments(const vog_copy_seg* segs, int n, void* stream) {
  using namespace vog;
  VOG_CHECK_ARG(n >= 0 && n <= VOG_MAX_COPY_SEGS && (n == 0 || segs));
  if (n == 0) return 0;
  CopySegs cs;
  size_t mx = 0;
  for (int i = 0; i < n; ++i) {
    VOG_CHECK_ARG(segs[i].src && segs[i].dst && ((uintptr_t)segs[i].src & 15) == 0 && ((uintptr_t)segs[i].dst & 15) == 0);
    cs.s[i] = segs[i];
    mx = segs[i].bytes > mx ? segs[i].bytes : mx;
  }
  size_t gx = (mx + 4095) / 4096;                          // one 16-byte chunk per thread for the largest segment ...
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);               // ... up to 1024 blocks (4 MB in flight per pass)
  ::vog::launch(copy_segments_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, cs);
  VOG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vog_assemble_batch(const vog_assemble_args* a, void* stream) {
  using namespace vog;
  VOG_CHECK_ARG(a && a->props_in && a->props_out && a->region_in && a->region_out && a->seg_in && a->seg_out);
  VOG_CHECK_ARG(a->conc_type == VOG_CONC_SPAT || a->conc_type == VOG_CONC_TEMP);
  VOG_CHECK_ARG(a->B > 0 && a->ncmp > 0 && a->ncmp <= 64 && a->nfrm0 > 0 && a->nppf0 > 0 &&
                (a->prop_dim % 4) == 0 && (a->seg_dim % 4) == 0);
  VOG_CHECK_ARG((a->pnt_in == nullptr) == (a->pnt_out == nullptr));
  const int64_t rows = (int64_t)a->B * a->ncmp * a->nfrm0 * (a->nppf0 + 1);
  ::vog::launch(assemble_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, *a);
  VOG_LAUNCH_CHECK();
  if (a->gt_in) {
    VOG_CHECK_ARG(a->gt_out && a->num_box && a->num_box_out && a->target_cmp && a->srl_boxes_in && a->srl_boxes_out &&
                  a->srl_boxes_lens && a->frm_out && a->G > 0 && a->G <= 1024 && a->nv > 0 && a->nsrl > 0 && a->nbox > 0);
    ::vog::launch(assemble_gt_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a);
    VOG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int vog_assemble_from_bank(const vog_bank_assemble_args* a, void* stream) {
  using namespace vog;
  VOG_CHECK_ARG(a && a->bank.region && a->bank.seg && a->bank.props && a->index && a->props_out && a->region_out && a->seg_out);
  VOG_CHECK_ARG(a->conc_type == VOG_CONC_SPAT || a->conc_type == VOG_CONC_TEMP || a->conc_type == VOG_CONC_SEP);
  VOG_CHECK_ARG(a->bank.feat_dtype == VOG_BANK_F32 || a->bank.feat_dtype == VOG_F16);
  const bool f16 = a->bank.feat_dtype == VOG_F16;
  const int q = f16 ? 8 : 4;                               // elements of a 16-byte load
  VOG_CHECK_ARG(a->bank.V > 0 && a->bank.V <= 0x7fffffffLL);
  VOG_CHECK_ARG(a->B > 0 && a->ncmp > 0 && a->ncmp <= 64 && a->nfrm0 > 0 && a->nppf0 > 0 && a->prop_dim > 0 && a->seg_dim > 0 &&
                (a->prop_dim % q) == 0 && (a->seg_dim % q) == 0);
  VOG_CHECK_ARG((((uintptr_t)a->bank.region | (uintptr_t)a->bank.seg | (uintptr_t)a->region_out | (uintptr_t)a->seg_out) & 15) == 0);
  VOG_CHECK_ARG(a->pnt_out == nullptr || a->bank.pnt != nullptr);
  const int64_t rows = (int64_t)a->B * a->ncmp * a->nfrm0 * (a->nppf0 + 1);
  VOG_CHECK_ARG(rows <= 0x7fffffffLL);
  if (f16) ::vog::launch(bank_rows_kernel<_Float16>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, *a);
  else ::vog::launch(bank_rows_kernel<float>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, *a);
  VOG_LAUNCH_CHECK();
  if (a->gt_out) {
    VOG_CHECK_ARG(a->bank.gt && a->bank.num_box && a->num_box_out && a->G > 0);
    if (a->conc_type == VOG_CONC_SEP) {
      VOG_CHECK_ARG(a->frm_out == nullptr || a->bank.pnt != nullptr);
      ::vog::launch(bank_gt_sep_kernel, dim3((unsigned)(a->B * a->ncmp)), dim3(256), 0, (hipStream_t)stream, *a);
    } else {
      VOG_CHECK_ARG(a->target_cmp && a->srl_boxes_in && a->srl_boxes_out && a->srl_boxes_lens && a->frm_out && a->G <= 1024 &&
                    a->nv > 0 && a->nsrl > 0 && a->nbox > 0);
      ::vog::launch(bank_gt_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a);
    }
    VOG_LAUNCH_CHECK();
  }
  return 0;
}
