// Whole-forward engine: weight registry, workspace plan, launch sequence,
// hipGraph capture. Replaces Conc{TEMP,SPAT,SEP}.forward
// (mdl_conc_single.py:68-127, mdl_conc_sep.py:131-217) and
// Evaluator*.get_out_results_boxes (eval_vsrl_corr.py:162-424) with ~50 kernel
// launches on caller-owned buffers; no allocation and no sync on the launch path.
#include <stdarg.h>
#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>
#include <stdlib.h>
#include "common.h"
#include "wpack_dev.h"

namespace vog {

// ---- error string -------------------------------------------------------------
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int attn_head_pad(int dh);
int attn_split_supported(int N, int dp);
int attn_struct_split_supported(int nppf, int nsrl, int dp);
int tx_tail_supported(int d, int dh, int kwo);
int tx_tail_split_supported(int d, int dh, int kwo);      // the widths with hi + lo bodies (512 / 768)
int64_t tx_tail_scratch_bytes(int M, int d);
int vis_encode_supported(int prop_dim, int seg_dim, int prop_enc, int seg_enc);
int vis_split_run(const float* c32, int64_t ldc, float* enc_prop, float* enc_seg, int n_rows, int nppf0, int prop_enc, int seg_enc,
                  hipStream_t st);
int logit_fold_run(const unsigned int* logit_max, unsigned int* stats, unsigned int* published, int n_stacks, hipStream_t st);
int pair_launch(const std::function<int(hipStream_t)>& fa, const std::function<int(hipStream_t)>& fb,
                hipStream_t st, bool* fused);
// mul_pl + vis_prep + vis_concat / obj_restore as one bank_prep grid (elementwise.hip)
int bank_prep_launch(const std::function<int(hipStream_t)>& f_gemm, const std::function<int(hipStream_t)>& f_prep,
                     const std::function<int(hipStream_t)>& f_rows, hipStream_t st);

// ---- host fp32 -> 16 bit ------------------------------------------------------
static unsigned short h_to16(float f, int dt) {
  if (dt == VOG_BF16) {
    unsigned int u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
  }
  _Float16 h = (_Float16)f;
  unsigned short r;
  memcpy(&r, &h, 2);
  return r;
}

struct TxLayer {
  unsigned short *wqkv, *wo, *w1, *w2;     // 16-bit, padded
  unsigned short* wqkv_lang_f;             // Wqkv[:, d_vis:] in fragment order (structured layer 0)
  unsigned short *wo_p, *w1_p, *w2_p;      // 32x16 fragment order (fused encoder tail, txtail.hip), or null
  unsigned short *wqkv_p, *wqkv_pv;        // padded Wqkv in the same order (all-columns QKV of p100, qkvrb_dev.h): all d columns / the first d_vis
  float *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
  // hi + lo operands (tx_split): 16-bit remainders t16(w - t16(w)) in the layouts of wqkv, wqkv_lang_f, wo_p, w1_p, w2_p
  unsigned short *wqkv_lo, *wqkv_lang_f_lo, *wo_p_lo, *w1_p_lo, *w2_p_lo;
};
struct TxWeights {
  int d = 0, H = 0, dp = 0, dh = 0, n_layers = 0, use_rel = 0;
  std::vector<int> head_off, head_dim;
  std::vector<TxLayer> layers;
  float *pe_w = nullptr, *pe_b = nullptr;
};

// One row of the image table: a device buffer vog_ctx_finalize made, and how it derives from the weights (wpack_dev.h).
// g carries the destination, its byte count and the geometry; its source pointers are filled per refresh.
struct WImage {
  std::string name;
  int kind;                             // vog_image_kind
  std::vector<std::string> srcs;        // source weight names, in the order of g.src (the gate table: its own order)
  WpackImage g;
};

}  // namespace vog

using namespace vog;

struct vog_ctx {
  vog_model_desc d;
  std::vector<WImage> images;           // every device buffer of `allocs`, in the order finalize made them
  std::set<std::string> stale;          // weights rewritten on the device since their host copy was set (vog_ctx_refresh_device)
  unsigned short* gx_wperm = nullptr;   // gate-table operands of a device refresh: permuted 16-bit W_ih_l0 and bias sums,
  float* gx_bperm = nullptr;            // allocated by the first refresh, kept until the context goes
  std::vector<std::string> names;                       // required weights
  std::map<std::string, int64_t> numel;
  std::map<std::string, std::vector<float>> host;
  std::vector<void*> allocs;
  bool finalized = false;
  int tx_split = 0;                     // round 6: hi + lo 16-bit operands (three MFMAs per product) for everything that feeds attention
                                        // logits - encoders, QKV projections, Q.K^T, and the tails whose output is another layer's
                                        // input: the plan for checkpoints whose attention is too sharp for 16-bit logits but does
                                        // not need the fp32 path (engine.py picks it from the weights; set before vog_ctx_finalize)
  unsigned short *w_prop_f_lo = nullptr, *w_seg_f_lo = nullptr;
  int lstm_inject_stall = 0;            // test hook: persistent layer launches behave as if their hand-off had timed out
  int lstm_persistent = 1;              // one launch per BiLSTM layer where supported (W_hh resident on chip; vog_hip.h)
  int lstm_wide = 0;                    // ... and for 17 .. 32 sentences too (vog_bilstm_layer_wide; opt-in)
  int fused_tail = 1;                   // Wo..LN2 (+ lin2 + score) of an encoder layer as one launch where supported
  // device weights
  float* emb = nullptr;
  unsigned short* emb16 = nullptr;                      // 16-bit copy: A operand when the LSTM input GEMM has M > 64
  std::vector<unsigned short*> wih;                     // [layer] [8R, in]
  std::vector<unsigned short*> wih_f;                   // same, fragment order (M <= 64 kernel)
  unsigned short* w_outproj_f = nullptr;
  std::vector<unsigned short*> whh;                     // [layer] [2][4R][R]
  std::vector<unsigned short*> wih_p;                   // [layer] W_ih in the W_hh tile order (fused input projection), or null
  int fused_ih = 1;                     // LSTM input projections inside the persistent layer kernel where supported (no GEMM
                                        // launches, no gx round trip; W_ih streams through the layer's 64 CUs: +7 / +17 us per
                                        // layer against 6.4 / 9.7 us whole-chip launches -> 5 % more throughput with 4 batches
                                        // in flight, 10 us more single-batch latency)
  std::vector<float*> bsum;                             // [layer] [8R]
  float* gx0_tab = nullptr;             // round 6: [vocab + 1][2][R][4 gates] fp32 = emb . W_ih_l0^T + b_ih + b_hh for every token and both directions
                                        // (vog_lstm_layer_args.gx_table): layer 0's gate inputs are a look-up, built once per checkpoint
  unsigned short *w_outproj = nullptr, *w_prop = nullptr, *w_seg = nullptr, *w_lin2 = nullptr;
  unsigned short* w_lin2_p = nullptr;                   // lin2.0 in 32x16 fragment order (fused score head)
  unsigned short *w_prop_f = nullptr, *w_seg_f = nullptr;   // encoder weights in 16x32 fragment order (visenc.hip)
  int fused_enc = 1;                    // both feature encoders + concat as one launch where supported
  int enc_lean = -1;                    // -1: lean form exactly when the encoders share a BiLSTM layer's launch
  int pair_launches = 1;                // step i of the language chain shares a launch with step i of the visual chain (pair.hip)
  int pair_mask = 15;                   // which pairs are formed: 1 BiLSTM layer 0 + encoders, 2 layer 1 + obj tail, 4 out-projection + mul QKV,
                                        // 8 layer-1 input projection (where it is a GEMM launch) + obj QKV
  float *b_outproj = nullptr, *b_prop = nullptr, *b_seg = nullptr, *b_lin2 = nullptr;
  float *w_arg = nullptr, *b_arg = nullptr, *w_lin2b = nullptr, *b_lin2b = nullptr;
  float *w_sv0 = nullptr, *b_sv0 = nullptr, *w_sv2 = nullptr, *b_sv2 = nullptr;
  TxWeights obj, mul;
  uint32_t* stats = nullptr;            // vog_ctx_set_stats: where vog_ctx_obj_videos publishes obj_tx's logit maxima
};

namespace vog {

static bool has_obj(const vog_model_desc& d) {
  return d.mdl_kind == VOG_MDL_VGRND || (d.mdl_kind == VOG_MDL_VOG && d.obj_to_use);
}
static bool has_obj_weights(const vog_model_desc& d) { return d.mdl_kind != VOG_MDL_IGRND; }
static bool has_mul(const vog_model_desc& d) { return d.mdl_kind == VOG_MDL_VOG; }

static void add_w(vog_ctx* c, const std::string& n, int64_t numel) {
  c->names.push_back(n);
  c->numel[n] = numel;
}

static void declare_tx(vog_ctx* c, const char* prefix, int d, int n_layers) {
  const int dh = d / 2;
  for (int l = 0; l < n_layers; ++l) {
    std::string p = std::string(prefix) + ".encoder.layers." + std::to_string(l);
    for (const char* w : {"wq", "wk", "wv", "wo"}) add_w(c, p + ".selfattn.layer." + w + ".weight", (int64_t)d * d);
    add_w(c, p + ".selfattn.layernorm.weight", d);
    add_w(c, p + ".selfattn.layernorm.bias", d);
    add_w(c, p + ".feedforward.layer.linear1.weight", (int64_t)dh * d);
    add_w(c, p + ".feedforward.layer.linear1.bias", dh);
    add_w(c, p + ".feedforward.layer.linear2.weight", (int64_t)d * dh);
    add_w(c, p + ".feedforward.layer.linear2.bias", d);
    add_w(c, p + ".feedforward.layernorm.weight", d);
    add_w(c, p + ".feedforward.layernorm.bias", d);
  }
}

template <typename T>
static int upload(vog_ctx* c, const std::vector<T>& h, T** out) {
  void* p = nullptr;
  VOG_HIP(hipMalloc(&p, h.size() * sizeof(T) + 64));
  c->allocs.push_back(p);
  VOG_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (T*)p;
  return 0;
}

static const std::vector<float>& W(vog_ctx* c, const std::string& n) { return c->host.at(n); }

// ---- image table ------------------------------------------------------------------------------------------
static WpackImage wimg(int layout, int view, int dt, int lo, int N, int64_t K, int64_t ld, int k0 = 0) {
  WpackImage g{};
  g.layout = layout; g.view = view; g.dt = dt; g.lo = lo; g.N = N; g.K = (int)K; g.ld = ld; g.k0 = k0;
  return g;
}
static void rec(vog_ctx* c, const std::string& name, int kind, void* dev, WpackImage g, std::vector<std::string> srcs) {
  g.dst = dev;
  g.bytes = (int64_t)g.N * g.K * (g.dt < 0 ? 4 : 2);
  c->images.push_back({name, kind, std::move(srcs), g});
}

// w - t16(w): what the second operand of a hi + lo product carries (exact in fp32)
static std::vector<float> remainder16(const float* w, size_t n, int dt) {
  std::vector<float> r(n);
  for (size_t i = 0; i < n; ++i) {
    const unsigned short h = h_to16(w[i], dt);
    float back;
    if (dt == VOG_BF16) { unsigned int u = (unsigned int)h << 16; memcpy(&back, &u, 4); }
    else { _Float16 f; memcpy(&f, &h, 2); back = (float)f; }
    r[i] = w[i] - back;
  }
  return r;
}

static std::vector<unsigned short> to16(const std::vector<float>& w, int dt) {
  std::vector<unsigned short> h(w.size());
  for (size_t i = 0; i < w.size(); ++i) h[i] = h_to16(w[i], dt);
  return h;
}

static int up32(vog_ctx* c, const std::string& n, float** out, const std::string& img) {
  VOG_TRY(upload<float>(c, W(c, n), out));
  rec(c, img, VOG_IMG_F32, *out, wimg(WL_PLAIN, WV_DIRECT, -1, 0, 1, (int64_t)W(c, n).size(), 0), {n});
  return 0;
}
static int up16(vog_ctx* c, const std::string& n, int dt, unsigned short** out, const std::string& img) {
  VOG_TRY(upload<unsigned short>(c, to16(W(c, n), dt), out));
  rec(c, img, VOG_IMG_CAST16, *out, wimg(WL_PLAIN, WV_DIRECT, dt, 0, 1, (int64_t)W(c, n).size(), 0), {n});
  return 0;
}

// fp32 [N, ld] host matrix -> 32x16 fragment order on the device (vog_pack_w_frag32)
static int up_frag32(vog_ctx* c, const float* w, int64_t ld, int N, int K, int dt, unsigned short** out) {
  std::vector<unsigned short> h((size_t)N * K);
  VOG_TRY(vog_pack_w_frag32(w, ld, N, K, h.data(), (vog_dtype)dt));
  return upload<unsigned short>(c, h, out);
}

static int finalize_tx(vog_ctx* c, const char* prefix, const char* pe_name, int d, int H,
                       int n_layers, int use_rel, TxWeights* tw) {
  const int dt = c->d.tx_dtype;
  tw->d = d; tw->H = H; tw->n_layers = n_layers; tw->use_rel = use_rel;
  const int chunk = (d + H - 1) / H;                     // torch.chunk: ceil(d/H), last shorter
  int off = 0;
  for (int h = 0; h < H; ++h) {
    const int sz = std::min(chunk, d - off);
    if (sz <= 0) VOG_FAIL(-1, "d_model %d cannot be chunked into %d heads", d, H);
    tw->head_off.push_back(off);
    tw->head_dim.push_back(sz);
    off += sz;
  }
  tw->dp = attn_head_pad(chunk);
  if (tw->dp < 0) VOG_FAIL(-1, "head dim %d > 256 unsupported", chunk);
  const int dp = tw->dp, dh = d / 2;
  tw->dh = dh;
  // head-padded views of Wq / Wk / Wv (rows) and Wo (columns): wpack_head_src, the map the device packer uses
  auto heads = [&](WpackImage g) { g.H = H; g.dp = dp; g.chunk = chunk; g.d = d; return g; };
  for (int l = 0; l < n_layers; ++l) {
    std::string p = std::string(prefix) + ".encoder.layers." + std::to_string(l);
    const std::string im = std::string(prefix) + "." + std::to_string(l) + ".";      // image names
    const std::vector<std::string> qkv_src = {p + ".selfattn.layer.wq.weight", p + ".selfattn.layer.wk.weight",
                                              p + ".selfattn.layer.wv.weight"};
    const std::string wo_n = p + ".selfattn.layer.wo.weight", w1_n = p + ".feedforward.layer.linear1.weight",
                      w2_n = p + ".feedforward.layer.linear2.weight";
    const int nq = 3 * H * dp, kwo = H * dp;
    TxLayer L{};
    // fp32 image of columns [k0, k0 + nk) of the padded [3 * H * dp, d] Wq / Wk / Wv (zero rows for the head padding)
    auto padded_qkv = [&](int k0, int nk) {
      std::vector<float> m((size_t)nq * nk, 0.f);
      for (int n = 0; n < nq; ++n) {
        const int r = wpack_head_src(n % kwo, H, dp, chunk, d);
        if (r >= 0) memcpy(&m[(size_t)n * nk], &W(c, qkv_src[n / kwo])[(size_t)r * d + k0], nk * sizeof(float));
      }
      return m;
    };
    const std::vector<float> wqf = padded_qkv(0, d);
    VOG_TRY(upload<unsigned short>(c, to16(wqf, dt), &L.wqkv));
    rec(c, im + "wqkv", VOG_IMG_QKV_PAD, L.wqkv, heads(wimg(WL_PLAIN, WV_QKV, dt, 0, nq, d, d)), qkv_src);
    // remainder of the padded [3*H*dp, d] weights, same plain layout
    if (c->tx_split) {
      VOG_TRY(upload<unsigned short>(c, to16(remainder16(wqf.data(), wqf.size(), dt), dt), &L.wqkv_lo));
      rec(c, im + "wqkv_lo", VOG_IMG_QKV_PAD, L.wqkv_lo, heads(wimg(WL_PLAIN, WV_QKV, dt, 1, nq, d, d)), qkv_src);
    }
    if (vog_qkv_rowblock_supported(nq, d)) {
      VOG_TRY(up_frag32(c, wqf.data(), d, nq, d, dt, &L.wqkv_p));
      rec(c, im + "wqkv_p", VOG_IMG_FRAG32, L.wqkv_p, heads(wimg(WL_FRAG32, WV_QKV, dt, 0, nq, d, d)), qkv_src);
    }
    const int dl = c->d.lang_enc, dv = d - dl;
    const bool mul_l0 = l == 0 && std::string(prefix) == "mult_txf" && dv > 0;
    if (mul_l0 && vog_qkv_rowblock_supported(nq, dv)) {
      VOG_TRY(up_frag32(c, wqf.data(), d, nq, dv, dt, &L.wqkv_pv));
      rec(c, im + "wqkv_pv", VOG_IMG_FRAG32, L.wqkv_pv, heads(wimg(WL_FRAG32, WV_QKV, dt, 0, nq, dv, d)), qkv_src);
    }
    if (mul_l0 && dl % 32 == 0) {
      // fp32 image of the padded lang columns, then fragment order
      const std::vector<float> wl = padded_qkv(dv, dl);
      std::vector<unsigned short> wf(wl.size());
      VOG_TRY(vog_pack_w_frag(wl.data(), dl, nq, dl, wf.data(), (vog_dtype)dt));
      VOG_TRY(upload<unsigned short>(c, wf, &L.wqkv_lang_f));
      rec(c, im + "wqkv_lang_f", VOG_IMG_FRAG16, L.wqkv_lang_f, heads(wimg(WL_FRAG16, WV_QKV, dt, 0, nq, dl, d, dv)), qkv_src);
      if (c->tx_split) {
        const std::vector<float> r = remainder16(wl.data(), wl.size(), dt);
        VOG_TRY(vog_pack_w_frag(r.data(), dl, nq, dl, wf.data(), (vog_dtype)dt));
        VOG_TRY(upload<unsigned short>(c, wf, &L.wqkv_lang_f_lo));
        rec(c, im + "wqkv_lang_f_lo", VOG_IMG_FRAG16, L.wqkv_lang_f_lo, heads(wimg(WL_FRAG16, WV_QKV, dt, 1, nq, dl, d, dv)), qkv_src);
      }
    }
    // the padded Wo as fp32 (zero columns for the head padding)
    std::vector<float> wof((size_t)d * kwo, 0.f);
    const auto& wo = W(c, wo_n);
    for (int o = 0; o < d; ++o)
      for (int k = 0; k < kwo; ++k) {
        const int cc = wpack_head_src(k, H, dp, chunk, d);
        if (cc >= 0) wof[(size_t)o * kwo + k] = wo[(size_t)o * d + cc];
      }
    VOG_TRY(upload<unsigned short>(c, to16(wof, dt), &L.wo));
    rec(c, im + "wo", VOG_IMG_WO_PAD, L.wo, heads(wimg(WL_PLAIN, WV_WO, dt, 0, d, kwo, d)), {wo_n});
    if (tx_tail_supported(d, dh, kwo)) {     // the same weights in fragment order (fused tail)
      const auto& w1 = W(c, w1_n);
      const auto& w2 = W(c, w2_n);
      VOG_TRY(up_frag32(c, wof.data(), (int64_t)kwo, d, kwo, dt, &L.wo_p));
      rec(c, im + "wo_p", VOG_IMG_FRAG32, L.wo_p, heads(wimg(WL_FRAG32, WV_WO, dt, 0, d, kwo, d)), {wo_n});
      VOG_TRY(up_frag32(c, w1.data(), d, dh, d, dt, &L.w1_p));
      rec(c, im + "w1_p", VOG_IMG_FRAG32, L.w1_p, wimg(WL_FRAG32, WV_DIRECT, dt, 0, dh, d, d), {w1_n});
      VOG_TRY(up_frag32(c, w2.data(), dh, d, dh, dt, &L.w2_p));
      rec(c, im + "w2_p", VOG_IMG_FRAG32, L.w2_p, wimg(WL_FRAG32, WV_DIRECT, dt, 0, d, dh, dh), {w2_n});
      if (c->tx_split) {
        VOG_TRY(up_frag32(c, remainder16(wof.data(), wof.size(), dt).data(), (int64_t)kwo, d, kwo, dt, &L.wo_p_lo));
        rec(c, im + "wo_p_lo", VOG_IMG_FRAG32, L.wo_p_lo, heads(wimg(WL_FRAG32, WV_WO, dt, 1, d, kwo, d)), {wo_n});
        VOG_TRY(up_frag32(c, remainder16(w1.data(), w1.size(), dt).data(), d, dh, d, dt, &L.w1_p_lo));
        rec(c, im + "w1_p_lo", VOG_IMG_FRAG32, L.w1_p_lo, wimg(WL_FRAG32, WV_DIRECT, dt, 1, dh, d, d), {w1_n});
        VOG_TRY(up_frag32(c, remainder16(w2.data(), w2.size(), dt).data(), dh, d, dh, dt, &L.w2_p_lo));
        rec(c, im + "w2_p_lo", VOG_IMG_FRAG32, L.w2_p_lo, wimg(WL_FRAG32, WV_DIRECT, dt, 1, d, dh, dh), {w2_n});
      }
    }
    VOG_TRY(up16(c, w1_n, dt, &L.w1, im + "w1"));
    VOG_TRY(up16(c, w2_n, dt, &L.w2, im + "w2"));
    VOG_TRY(up32(c, p + ".feedforward.layer.linear1.bias", &L.b1, im + "b1"));
    VOG_TRY(up32(c, p + ".feedforward.layer.linear2.bias", &L.b2, im + "b2"));
    VOG_TRY(up32(c, p + ".selfattn.layernorm.weight", &L.ln1g, im + "ln1g"));
    VOG_TRY(up32(c, p + ".selfattn.layernorm.bias", &L.ln1b, im + "ln1b"));
    VOG_TRY(up32(c, p + ".feedforward.layernorm.weight", &L.ln2g, im + "ln2g"));
    VOG_TRY(up32(c, p + ".feedforward.layernorm.bias", &L.ln2b, im + "ln2b"));
    tw->layers.push_back(L);
  }
  VOG_TRY(up32(c, std::string(pe_name) + ".weight", &tw->pe_w, std::string(prefix) + ".pe_w"));
  VOG_TRY(up32(c, std::string(pe_name) + ".bias", &tw->pe_b, std::string(prefix) + ".pe_b"));
  return 0;
}

// ---- geometry + workspace plan ---------------------------------------------------
struct Geo {
  int B, ncmp, T, sep, nvl, nc_v, nfrm, nppf, NP, Fv, n_vid, Bn, Bn16, R, E, L, d_obj, d_mul;
  int S_obj, N_obj, spv_obj, npad_obj; float fdiv_obj;
  int S_mul, N_mul, npad_mul;
  int64_t rows_obj, rows_mul;
};

static Geo make_geo(const vog_model_desc& d, int B, int ncmp, int T) {
  Geo g{};
  g.B = B; g.ncmp = ncmp; g.T = T;
  g.sep = d.conc_type == VOG_CONC_SEP;
  g.nvl = g.sep ? ncmp : 1;
  g.nc_v = g.sep ? ncmp : 1;
  g.nfrm = d.conc_type == VOG_CONC_TEMP ? ncmp * d.nfrm0 : d.nfrm0;
  g.nppf = d.conc_type == VOG_CONC_SPAT ? ncmp * d.nppf0 : d.nppf0;
  g.NP = g.nfrm * g.nppf;
  g.Fv = g.NP / d.nppf0;
  g.n_vid = B * g.nc_v;
  g.Bn = B * g.nvl;
  g.Bn16 = (int)round_up64(g.Bn, 16);
  g.R = d.rnn_size; g.E = d.emb_dim; g.L = d.lang_enc;
  g.d_obj = d.prop_enc + d.seg_enc;
  g.d_mul = g.d_obj + d.lang_enc;
  g.S_obj = d.obj_one_frm ? g.n_vid * g.nfrm : g.n_vid;
  g.N_obj = d.obj_one_frm ? g.nppf : g.NP;
  g.spv_obj = d.obj_one_frm ? g.nfrm : 1;
  g.fdiv_obj = d.obj_one_frm ? (float)g.nfrm : 1.0f;
  g.npad_obj = (int)round_up64(g.N_obj, 32);
  g.S_mul = g.n_vid * g.nfrm;
  g.N_mul = d.nsrl * g.nppf;
  g.npad_mul = (int)round_up64(g.N_mul, 32);
  g.rows_obj = (int64_t)g.n_vid * g.NP;
  g.rows_mul = (int64_t)g.S_mul * g.N_mul;
  return g;
}

struct Plan {
  std::map<std::string, std::pair<int64_t, int64_t>> buf;   // name -> (offset, bytes)
  int64_t total = 0;
  int64_t zero_off = 0, zero_bytes = 0, ones_off = 0, ones_bytes = 0;
  int64_t add(const std::string& n, int64_t bytes) {
    const int64_t off = total;
    buf[n] = {off, bytes};
    total += round_up64(bytes, 256);
    return off;
  }
};

static Plan make_plan(const vog_ctx* c, const Geo& g, bool lang_only = false) {
  const vog_model_desc& d = c->d;
  Plan p;
  const int nl = d.rnn_layers;
  p.add("logit_pub", 256);                            // the logit maxima this workspace's forwards last published to the host
                                                      // (vog_pred_args.published; zeroed with the workspace, not per forward)
  p.add("logit_max", 2 * 4 * VOG_LOGIT_WORDS * VOG_LOGIT_STRIDE * 4);   // [2 stacks][4 layers][words, 128 B apart]: the running largest
                                                      // |attention logit| of this workspace's forwards (float bits; raise-only, zeroed
                                                      // with the workspace)
  // ---- zero-initialised region (one memset per forward)
  p.zero_off = p.total;
  for (int l = 0; l < nl; ++l) {
    // out16 of layer l is followed directly by the h buffer that holds the FINAL
    // state, so [out16 ; h_final] is one contiguous A operand for the out-proj GEMM
    // (hA lives inside the same allocation: rows [Bn*T, Bn*T + Bn16) )
    p.add("lstm_out16_" + std::to_string(l), (int64_t)(round_up64(g.Bn * g.T + g.Bn, 16) + g.Bn16) * 2 * g.R * 2);
    p.add("lstm_hB_" + std::to_string(l), (int64_t)g.Bn16 * 2 * g.R * 2);
    p.add("lstm_hA2_" + std::to_string(l), (int64_t)g.Bn16 * 2 * g.R * 2);   // ping buffer when out16 is fragment-ordered
    p.add("lstm_c_" + std::to_string(l), (int64_t)g.Bn16 * 2 * g.R * 4);
    p.add("lstm_sync_" + std::to_string(l), 1024);   // [2] timeout, [16 + 16 dir + xcc] workgroups arrived per XCC id
  }
  p.add("obj_guard", 256);                            // vog_attn_args.guard_flag of the two stacks (long-sequence attention): zeroed
  p.add("mul_guard", 256);                            // with the rest of this region, so the attention needs no clearing launch
  p.add("mul_ef_guard", 256);                         // vog_attn_struct_args.guard_flag (E x F attention of mul_tx layer 0, p100)
  p.zero_bytes = p.total - p.zero_off;
  // ---- 0xff-initialised region, directly behind the zeros (same fill loop of the prologue): the
  // hand-off slots of the persistent BiLSTM, [T][2][Bn][R] 16-bit per layer (lstm_dev.h)
  p.ones_off = p.total;
  for (int l = 0; l < nl; ++l) p.add("lstm_hx_" + std::to_string(l), vog_bilstm_hx_bytes(g.Bn, g.T, g.R));
  p.ones_bytes = p.total - p.ones_off;
  p.add("emb_a0", round_up64(g.Bn * g.T, 16) * g.E * 2);   // layer-0 A operand in fragment order (M <= 64)
  p.add("tok", (int64_t)g.Bn * g.T * 4);
  p.add("lstm_rows", (int64_t)2 * g.Bn * g.T * 4);
  p.add("gx", (int64_t)g.Bn * g.T * 8 * g.R * 4);
  p.add("full", (int64_t)(g.Bn * g.T + g.Bn16) * g.L * 4);
  p.add("lang", (int64_t)g.Bn * d.nsrl * g.L * 4);
  p.add("outproj_slabs", (int64_t)8 * (g.Bn * g.T + g.Bn) * g.L * 4);
  if (lang_only) return p;
  p.add("prop16", g.rows_obj * d.prop_dim * 2);
  p.add("seg16", (int64_t)g.n_vid * g.Fv * d.seg_dim * 2);
  p.add("enc_slabs", (int64_t)16 * (g.rows_obj * d.prop_enc + (int64_t)g.n_vid * g.Fv * d.seg_enc) * 4);
  p.add("prop_seg", g.rows_obj * g.d_obj * 4);
  p.add("prop_seg16", g.rows_obj * g.d_obj * 2);
  if (c->tx_split) p.add("prop_seg16_lo", g.rows_obj * g.d_obj * 2);
  auto tx = [&](const char* nm, const TxWeights& tw, int64_t rows, int S, int npad) {
    const std::string n(nm);
    if (c->tx_split) {     // 16-bit remainders of Q / K, of the attention rows and of the layer outputs (hi + lo operands)
      p.add(n + "_q_lo", (int64_t)S * tw.H * tw.dp * npad * 2);
      p.add(n + "_k_lo", (int64_t)S * tw.H * tw.dp * npad * 2);
      p.add(n + "_attn16_lo", rows * tw.H * tw.dp * 2);
      p.add(n + "_outA16_lo", rows * tw.d * 2);
      if (tw.n_layers > 1) p.add(n + "_outB16_lo", rows * tw.d * 2);
    }
    p.add(n + "_u", g.rows_obj * tw.H * 4);
    p.add(n + "_q", (int64_t)S * tw.H * tw.dp * npad * 2);      // fragment order, npad = N up to 32
    p.add(n + "_k", (int64_t)S * tw.H * tw.dp * npad * 2);
    p.add(n + "_vt", (int64_t)S * tw.H * tw.dp * npad * 2);
    p.add(n + "_attn16", rows * tw.H * tw.dp * 2);
    p.add(n + "_tmp", rows * tw.d * 4);
    p.add(n + "_x1", rows * tw.d * 4);
    p.add(n + "_x1_16", rows * tw.d * 2);
    p.add(n + "_ffn16", rows * tw.dh * 2);
    p.add(n + "_outA", rows * tw.d * 4);
    p.add(n + "_outA16", rows * tw.d * 2);
    p.add(n + "_x1s", tx_tail_scratch_bytes((int)rows, tw.d) + 16);
    if (tw.n_layers > 1) {
      p.add(n + "_outB", rows * tw.d * 4);
      p.add(n + "_outB16", rows * tw.d * 2);
    }
  };
  if (has_obj(d)) tx("obj", c->obj, g.rows_obj, g.S_obj, g.npad_obj);
  p.add("xmul", g.rows_mul * g.d_mul * 4);
  p.add("xmul16", g.rows_mul * g.d_mul * 2);
  if (has_mul(d)) {
    tx("mul", c->mul, g.rows_mul, g.S_mul, g.npad_mul);
    p.add("mul_pv", g.rows_obj * 3 * c->mul.H * c->mul.dp * 4);
    p.add("mul_pl", (int64_t)g.Bn * d.nsrl * 3 * c->mul.H * c->mul.dp * 4);
  }
  p.add("h1", g.rows_mul * 256 * 4);
  return p;
}

// The chain a step belongs to. The language chain and the visual (+ joint) chain are independent until mul_tx's attention,
// which is what lets step i of one share a launch with step i of the other (pair_pass); the prologue runs before both.
enum class Chain { Prologue, Language, Visual };
struct Step {
  std::string name;
  std::function<int(hipStream_t)> fn;
  Chain chain = Chain::Visual;
};

static int run_steps(const std::vector<Step>& steps, hipStream_t st) {
  for (auto& s : steps) VOG_TRY(s.fn(st));
  return 0;
}

struct WS {
  char* base; const Plan* plan;
  template <typename T> T* at(const std::string& n) const {
    return reinterpret_cast<T*>(base + plan->buf.at(n).first);
  }
};

// ---- the form of the BiLSTM chain, decided once per (context, geometry) -------------------------------
// Input projection inside the persistent layer kernel (no GEMM launch, no gx round trip): needs the layer input in fragment
// order (embedding rows from the prologue / the previous layer's out16), up to 80 (sentence, position) columns.
// fused_ih: 1 = every layer in the kernel where its prologue reaches, layer 0 by table look-up where it does not; 4 = the same
// without the table (GEMM launches beyond 80 columns); 5 = the table wherever the checkpoint has one; 2 = layer 0 only,
// 3 = layers >= 1 only (experiments), 0 = GEMM launches
constexpr int kMaxRnnLayers = 8;          // (vog_ctx_create)
struct LstmForm {
  bool persistent;                      // one launch per layer (vog_bilstm_layer) instead of T step launches
  bool wide;                            // ... the launch is vog_bilstm_layer_wide (17 .. 32 sentences, "lstm_wide"): never fused, never paired
  bool use_table;                       // layer 0 reads its gate inputs from the checkpoint's gate table (no input projection at all)
  bool emb_frag;                        // layer-0 A operand: the prologue gathers the embedding rows, 16 bit, in fragment order
  bool ih_fused[kMaxRnnLayers];         // layer l projects its input in its own kernel
  bool out_frag[kMaxRnnLayers];         // layer l writes out16 in A-fragment order
};

static LstmForm make_lstm_form(const vog_ctx* c, const Geo& g) {
  const int nl = c->d.rnn_layers, cols = g.Bn * g.T, mode = c->fused_ih;
  LstmForm f{};
  f.wide = c->lstm_persistent && c->lstm_wide && vog_bilstm_layer_wide_supported(g.Bn, g.R);
  f.persistent = f.wide || (c->lstm_persistent && vog_bilstm_layer_supported(g.Bn, g.R));
  // the embedding rows in fragment order: what the M <= 64 GEMM and layer 0's in-kernel projection read
  const bool emb_rows = cols <= vog_bilstm_fused_cols() && c->emb16 && (g.E % 32) == 0;
  // layer-0 gate inputs read from the checkpoint's gate table by the layer kernel itself (no input projection for layer 0 at all)
  // Used where the in-kernel projection does not reach (Bn x T > 80 columns: cfg 3, cfg 5, grouped / batched requests): there it
  // replaces a GEMM launch and the gate round trip (cfg 3 +2.3 %, cfg 5 +4.7 ... 7 %). Where the layer kernel can project in its
  // prologue (cfg 2) the two forms measured EQUAL (63.3 vs 63.5 k queries/s: the table reads are not quite hidden, 29.8 vs 30.7 us
  // for the layer) and the prologue, whose operands are always cache-resident, stays. fused_ih = 5: the table wherever it exists.
  const bool fuse0_ok = f.persistent && !f.wide && !c->wih_p.empty() && c->wih_p[0] && (g.E % 256) == 0 && emb_rows;
  f.use_table = c->gx0_tab && ((mode == 1 && !fuse0_ok) || mode == 5) && f.persistent && cols <= (f.wide ? 32 : 16) * 24;
  f.emb_frag = !f.use_table && emb_rows;
  auto can_fuse = [&](int l) {
    if (l >= nl || !f.persistent || f.wide || (l == 0 && f.use_table)) return false;
    const bool wanted = mode == 1 || mode == 4 || mode == 5 || (mode == 2 && l == 0) || (mode == 3 && l > 0);
    return wanted && c->wih_p[l] && ((l == 0 ? g.E : 2 * g.R) % 256) == 0 && cols <= vog_bilstm_fused_cols() && (l > 0 || emb_rows);
  };
  // LSTM outputs that feed M <= 64 GEMMs (next layer's input projection, final projection) or the next layer's in-kernel
  // projection are written in A-fragment order: those consumers load contiguous fragments
  const bool small = (cols + g.Bn) <= 64;
  for (int l = 0; l < nl; ++l) {
    f.out_frag[l] = small || can_fuse(l + 1);
    f.ih_fused[l] = can_fuse(l) && (l == 0 || f.out_frag[l - 1]);
  }
  return f;
}

// ---- transformer stacks (a7-a9) ---------------------------------------------------------------------------
// What a stack reads and what it leaves behind. hi + lo operands (c->tx_split): x16_lo / vis16_lo are the remainders of the
// stack's input rows / of the visual rows (structured layer 0), out16_lo the remainder of the 16-bit output copy.
struct TxStackIO {
  const float* x32; const void *x16, *x16_lo;     // the stack's input rows
  const void *vis16, *vis16_lo;                   // visual rows of the structured layer 0
  int S, N, npad, seq_per_vid, n_box;
  int last_dt;                                    // type of the LAST layer's 16-bit output copy (< 0: none is written)
  bool last_needs_f32;                            // somebody reads the last layer's fp32 output
  const vog_vislang_args* structured;             // layer 0 reads the [vis || lang] token structure instead of materialised rows
  const vog_score_args* score;                    // the last layer's fused tail may run lin2 + the score head
  bool out_feeds_attn;                            // the LAST layer's output is another attention layer's input (obj_tx under mul_tx)
  // results
  const float* out32; const void *out16, *out16_lo;
  bool score_done;                                // lin2 + score already ran inside the last tail
};

// one layer of a stack while its steps are built
struct TxLayerIO {
  const TxWeights& tw; const TxLayer& L; const std::string& n; int l; vog_dtype dt; int64_t rows;
  bool fact, last;                                // fact: structured layer 0 of mul_tx
  bool tail_split;                                // hi + lo tail: this layer's output is read by another attention layer
  const float* cur32; const void *cur16, *cur16_lo;
  float* u; unsigned int* lmax;
  void *attn16, *attn16_lo;
  float* o32; void *o16, *o16_lo;                 // this layer's output buffers
  float* o32w; void* o16w; vog_dtype odt;         // ... and which of them it writes, the 16-bit copy in which type
};

// ---- the step builder -----------------------------------------------------------------------------------
// What every stage needs, each flag decided once; the stages are its member functions and append to `steps`. A launch closure
// outlives the builder: it names what it captures (resolved pointers and values), never `this`.
struct Builder {
  const vog_ctx* const c;
  const vog_batch* const b;
  const vog_model_desc& d;
  const Geo& g;
  const WS ws;
  std::vector<Step>& steps;
  const bool lang_only;        // just the language chain of `b` (group encoder): the workspace is the language-only plan
  const bool shared;           // the language chain is NOT run: argument vectors come from a group encoder's workspace
  const bool structured;       // mul_tx consumes the [vis || lang] token structure directly (layer-0 QKV and its residual)
  // the language and the visual prologue are independent: one launch for both (not in the group forms, where they live in
  // different programs)
  const bool fuse_prep;
  const bool enc_fused;        // one launch for both encoders + the concat, straight from the fp32 features (visenc.hip)
  const bool encoded;          // the encoder outputs come with the batch (vog_batch.enc_prop / enc_seg): no encoder stage, nothing
                               // reads the raw feature pointers
  const bool cached_obj;       // obj_tx's output rows come with the batch (vog_batch.obj_out + enc_seg): nothing below mul_tx runs but
                               // the box-bias precursors of mul_tx and one obj_restore launch
  const bool pairs_possible;   // the pair pass runs (pair_pass; timing a step on its own switches it off)
  const bool bank_fuse;        // a forward served entirely from banks: its three-launch prologue may become one (bank_prep_pass)
  const LstmForm lstm;
  float* const lang_vec;

  Builder(const vog_ctx* c_, const vog_batch* b_, const Geo& g_, const WS& ws_, std::vector<Step>& steps_, bool lang_only_,
          bool allow_pairs)
      : c(c_), b(b_), d(c_->d), g(g_), ws(ws_), steps(steps_), lang_only(lang_only_),
        shared(!lang_only_ && b_->shared_lang != nullptr),
        structured(has_mul(c_->d) && (g_.d_obj % 64) == 0 && (g_.L % 32) == 0 && g_.rows_obj > 64),
        fuse_prep(!shared && !lang_only_),
        enc_fused(c_->fused_enc && c_->w_prop_f && c_->w_seg_f && !lang_only_),
        encoded(!lang_only_ && b_->enc_prop != nullptr),
        cached_obj(!lang_only_ && b_->obj_out != nullptr),
        pairs_possible(allow_pairs && c_->pair_launches && !shared && c_->lstm_persistent && !make_lstm_form(c_, g_).wide),
        bank_fuse(allow_pairs && c_->pair_launches && shared && (encoded || cached_obj) && structured && !c_->tx_split),
        lstm(make_lstm_form(c_, g_)),
        lang_vec(shared ? const_cast<float*>(b_->shared_lang) : ws_.at<float>("lang")) {}

  void add(Chain chain, const std::string& name, std::function<int(hipStream_t)> fn) { steps.push_back({name, std::move(fn), chain}); }
  void lang(const std::string& name, std::function<int(hipStream_t)> fn) { add(Chain::Language, name, std::move(fn)); }
  void vis(const std::string& name, std::function<int(hipStream_t)> fn) { add(Chain::Visual, name, std::move(fn)); }

  // fused visual prologue: raw features -> encoder operand type (the LDS-DMA GEMM cannot
  // convert in flight) + the box-bias precursors of both transformers
  vog_visprep_args visprep_args() {
    vog_visprep_args vp{};
    if (!enc_fused && !encoded && !cached_obj) {
      vp.src0 = b->pad_region_feature; vp.dst0 = ws.at<void>("prop16"); vp.n0 = g.rows_obj * d.prop_dim;
      vp.src1 = b->seg_feature_for_frms; vp.dst1 = ws.at<void>("seg16"); vp.n1 = (int64_t)g.n_vid * g.Fv * d.seg_dim;
    }
    vp.dtype = (vog_dtype)d.enc_dtype; vp.props = b->pad_proposals; vp.n_rows = (int)g.rows_obj; vp.vid_w = d.vid_w; vp.vid_h = d.vid_h;
    if (has_obj(d) && c->obj.use_rel && !cached_obj) {      // (cached rows: obj_tx does not run, w_pe0 stays NULL)
      vp.w_pe0 = c->obj.pe_w; vp.u0 = ws.at<float>("obj_u"); vp.H0 = c->obj.H; vp.nfrm_div0 = g.fdiv_obj;
    }
    if (has_mul(d) && c->mul.use_rel) {
      vp.w_pe1 = c->mul.pe_w; vp.u1 = ws.at<float>("mul_u"); vp.H1 = c->mul.H; vp.nfrm_div1 = (float)g.nfrm;
    }
    return vp;
  }

  // ---- language chain (a14-a16) ---------------------------------------------------------------------------
  void prologue_step() {
    char* z = ws.base + ws.plan->zero_off;
    const int64_t zb = ws.plan->zero_bytes, ob = ws.plan->ones_bytes;   // (the 0xff region starts where the zeros end)
    int32_t* tok = ws.at<int32_t>("tok");
    int32_t* lrows = ws.at<int32_t>("lstm_rows");
    const int64_t *wi = b->srl_arg_words_ind, *wm = b->srl_arg_word_mask, *lens = b->srl_arg_word_mask_len;
    const int nsrl = d.nsrl, sl = d.seq_len, V = d.vocab_size, Bn = g.Bn, T = g.T, E = g.E;
    const void* e16 = c->emb16;
    void* a0 = lstm.emb_frag ? ws.at<void>("emb_a0") : nullptr;
    if (fuse_prep) {
      const vog_visprep_args vp = visprep_args();
      add(Chain::Prologue, "prep", [z, zb, ob, wi, wm, lens, tok, lrows, Bn, T, nsrl, sl, V, e16, a0, E, vp](hipStream_t st) {
        return vog_prep_fused(z, zb, ob, wi, wm, lens, tok, lrows, Bn, T, nsrl, sl, V, e16, a0, E, &vp, st); });
    } else {
      lang("lang_prep", [z, zb, ob, wi, wm, lens, tok, lrows, Bn, T, nsrl, sl, V, e16, a0, E](hipStream_t st) {
        return vog_lang_prep(z, zb, ob, wi, wm, lens, tok, lrows, Bn, T, nsrl, sl, V, e16, a0, E, st); });
    }
  }

  // layer l of the BiLSTM: its input projection where that is a launch of its own, then one persistent launch or T steps
  void lstm_layer_steps(int l) {
    const LstmForm& f = lstm;
    const vog_dtype et = (vog_dtype)d.enc_dtype;
    const int R = g.R, T = g.T, Bn = g.Bn;
    const std::string sl = std::to_string(l);
    float* gx = ws.at<float>("gx");
    int32_t* tok = ws.at<int32_t>("tok");
    const bool ofrag = f.out_frag[l], table = l == 0 && f.use_table;
    vog_gemm_args ga{}; ga.c16_dtype = -1;
    if (l == 0) {
      ga.a = c->emb; ga.a_is_f32 = 1; ga.lda = g.E; ga.a_rows = tok; ga.K = g.E;
      // M > 64 runs on the LDS-DMA kernel, which cannot convert in flight: same values, pre-rounded
      if (Bn * T > 64 && c->emb16 && (g.E % 64) == 0) { ga.a = c->emb16; ga.a_is_f32 = 0; }
      // M <= 64: the prologue already gathered the rows, 16 bit, in fragment order
      if (Bn * T <= 64 && f.emb_frag) { ga.a = ws.at<void>("emb_a0"); ga.a_is_f32 = 0; ga.a_rows = nullptr; ga.a_frag = 1; }
    } else {
      ga.a = ws.at<void>("lstm_out16_" + std::to_string(l - 1)); ga.lda = 2 * R; ga.K = 2 * R;
      ga.a_frag = f.out_frag[l - 1] ? 1 : 0;      // (only read when this layer's projection is NOT in its kernel: then M <= 64)
    }
    // output rows land in (direction, step) order: gxs[dir][step][b][4R]
    ga.w = c->wih[l]; ga.ldw = ga.K; ga.bias = c->bsum[l]; ga.c32 = gx; ga.ldc = 4 * R;
    ga.M = Bn * T; ga.N = 8 * R; ga.rep = 1; ga.dtype = et;
    ga.out_rows = ws.at<int32_t>("lstm_rows"); ga.out_rows_ncol = 4 * R;
    if (ga.M <= 64 && c->wih_f[l]) { ga.w = c->wih_f[l]; ga.w_frag = 1; }
    if (!f.ih_fused[l] && !table) lang("lstm_ih" + sl, [ga](hipStream_t st) { return vog_gemm_bias_act(&ga, st); });
    if (f.persistent) {
      vog_lstm_layer_args pa{};
      pa.gxs = gx; pa.whh = c->whh[l]; pa.hx = ws.at<void>("lstm_hx_" + sl); pa.sync = ws.at<uint32_t>("lstm_sync_" + sl);
      pa.out16 = ws.at<void>("lstm_out16_" + sl);
      pa.lens = b->srl_arg_word_mask_len; pa.Bn = Bn; pa.T = T; pa.R = R; pa.dtype = et; pa.out_frag = ofrag ? 1 : 0;
      pa.fault = b->fault; pa.inject_stall = c->lstm_inject_stall;
      if (table) { pa.gx_table = c->gx0_tab; pa.tok = tok; }
      if (f.ih_fused[l]) {
        pa.wih = c->wih_p[l]; pa.bias = c->bsum[l]; pa.K = l == 0 ? g.E : 2 * R;
        pa.xa = l == 0 ? ws.at<void>("emb_a0") : ws.at<void>("lstm_out16_" + std::to_string(l - 1));
      }
      if (f.wide) lang("lstm_layer", [pa](hipStream_t st) { return vog_bilstm_layer_wide(&pa, st); });
      else lang("lstm_layer", [pa](hipStream_t st) { return vog_bilstm_layer(&pa, st); });
      return;
    }
    // final state must land in hA (adjacent to out16): after T steps it is in buf[T % 2]
    void* hA = ofrag ? ws.at<void>("lstm_hA2_" + sl)
                     : (void*)(ws.at<unsigned short>("lstm_out16_" + sl) + (int64_t)Bn * T * 2 * R);
    void* hB = ws.at<void>("lstm_hB_" + sl);
    void* hb[2] = {(T % 2) == 0 ? hA : hB, (T % 2) == 0 ? hB : hA};
    for (int s = 0; s < T; ++s) {
      vog_lstm_step_args la{};
      la.gx = gx; la.whh = c->whh[l]; la.h_in = hb[s % 2]; la.h_out = hb[(s + 1) % 2];
      la.c = ws.at<float>("lstm_c_" + sl); la.out16 = ws.at<void>("lstm_out16_" + sl);
      la.lens = b->srl_arg_word_mask_len; la.Bn = Bn; la.T = T; la.R = R; la.step = s; la.dtype = et;
      la.out_frag = ofrag ? 1 : 0; la.final_row0 = Bn * T;
      lang("lstm_step", [la](hipStream_t st) { return vog_bilstm_step(&la, st); });
    }
  }

  // lstm_out_feat_proj over [out16 ; h_final] of the top layer -> `full`
  void outproj_steps() {
    const int R = g.R;
    vog_gemm_args po{}; po.c16_dtype = -1;
    po.a = ws.at<void>("lstm_out16_" + std::to_string(d.rnn_layers - 1)); po.lda = 2 * R;
    po.w = c->w_outproj; po.ldw = 2 * R; po.bias = c->b_outproj; po.relu = 1;
    po.c32 = ws.at<float>("full"); po.ldc = g.L; po.M = g.Bn * g.T + g.Bn; po.N = g.L; po.K = 2 * R;
    po.rep = 1; po.dtype = (vog_dtype)d.enc_dtype;
    if (po.M <= 64 && c->w_outproj_f) { po.w = c->w_outproj_f; po.w_frag = 1; }
    po.a_frag = lstm.out_frag[d.rnn_layers - 1] ? 1 : 0;
    if (po.M > 64 && (po.K % 512) == 0 && (g.L % 4) == 0) {
      // few output tiles (L = 256 columns), long K: split K over 8 slabs, bias + ReLU in the finish
      vog_gemm_args ps = po; ps.bias = nullptr; ps.relu = 0; ps.c32 = ws.at<float>("outproj_slabs"); ps.splitk = 8;
      ps.w_frag = 0; ps.a_frag = 0; ps.w = c->w_outproj; ps.ldw = 2 * R;
      lang("lstm_outproj", [ps](hipStream_t st) { return vog_gemm_bias_act(&ps, st); });
      vog_splitk_prob f0{};
      f0.slabs = ps.c32; f0.splits = 8; f0.M = po.M; f0.N = g.L; f0.bias = c->b_outproj; f0.relu = 1; f0.rep = 1;
      f0.c32 = po.c32; f0.ldc = g.L;
      lang("lstm_outproj_finish", [f0](hipStream_t st) { return vog_splitk_finish(&f0, nullptr, st); });
    } else {
      lang("lstm_outproj", [po](hipStream_t st) { return vog_gemm_bias_act(&po, st); });
    }
  }

  int language_steps() {
    prologue_step();
    for (int l = 0; l < d.rnn_layers; ++l) lstm_layer_steps(l);
    outproj_steps();
    const float* full = ws.at<float>("full");
    float* lang_out = lang_vec;
    const int64_t *cap = b->srl_arg_words_capture, *im = b->srl_arg_inds_msk;
    const float *wa = c->w_arg, *ba = c->b_arg;
    const int Bn = g.Bn, T = g.T, nsrl = d.nsrl, L = g.L;
    lang("argvec", [full, cap, im, wa, ba, lang_out, Bn, T, nsrl, L](hipStream_t st) {
      return vog_srl_argvec(full, cap, im, wa, ba, lang_out, Bn, T, nsrl, L, st); });
    return 0;
  }

  // language half of mul_tx's layer-0 QKV: depends on `lang` only, so it rides on the language chain
  int mul_lang_proj_step() {
    const TxWeights& tw = c->mul;
    const TxLayer& L0 = tw.layers[0];
    const int ncol = 3 * tw.H * tw.dp;
    vog_gemm_args gl{}; gl.c16_dtype = -1;
    gl.a = lang_vec; gl.a_is_f32 = 1; gl.lda = g.L; gl.w = L0.wqkv + g.d_obj; gl.ldw = tw.d;
    gl.c32 = ws.at<float>("mul_pl"); gl.ldc = ncol; gl.M = g.Bn * d.nsrl; gl.N = ncol; gl.K = g.L;
    gl.rep = 1; gl.dtype = (vog_dtype)d.tx_dtype;
    if (gl.M <= 64 && L0.wqkv_lang_f) { gl.w = L0.wqkv_lang_f; gl.ldw = g.L; gl.w_frag = 1; }
    if (!c->tx_split) {
      lang("mul_pl", [gl](hipStream_t st) { return vog_gemm_bias_act(&gl, st); });
      return 0;
    }
    // hi + lo operands: the M <= 64 kernel carries them; more than 64 (sentence, argument) rows go through it 64 at a time
    if (!L0.wqkv_lang_f || !L0.wqkv_lang_f_lo) VOG_FAIL(-5, "tx_split: lang_enc %% 32 != 0");
    gl.w = L0.wqkv_lang_f; gl.ldw = g.L; gl.w_frag = 1; gl.w_lo = L0.wqkv_lang_f_lo;
    const int Mall = gl.M;
    lang("mul_pl", [gl, Mall](hipStream_t st) {
      for (int m0 = 0; m0 < Mall; m0 += 64) {
        vog_gemm_args g2 = gl;
        g2.a = (const float*)gl.a + (int64_t)m0 * gl.lda; g2.c32 = gl.c32 + (int64_t)m0 * gl.ldc;
        g2.M = Mall - m0 < 64 ? Mall - m0 : 64;
        VOG_TRY(vog_gemm_bias_act(&g2, st));
      }
      return 0; });
    return 0;
  }

  // ---- visual encoders (a12, a13) -------------------------------------------------------------------------
  // both encoders + the concat as one launch (visenc.hip)
  void fused_encoder_steps() {
    vog_visenc_args ve{};
    ve.prop = b->pad_region_feature; ve.seg = b->seg_feature_for_frms;
    ve.w_prop_f = c->w_prop_f; ve.w_seg_f = c->w_seg_f; ve.b_prop = c->b_prop; ve.b_seg = c->b_seg;
    ve.c32 = ws.at<float>("prop_seg"); ve.c16 = ws.at<void>("prop_seg16"); ve.ldc = g.d_obj; ve.c16_dtype = d.tx_dtype;
    ve.n_prop_rows = (int)g.rows_obj; ve.nppf0 = d.nppf0; ve.prop_dim = d.prop_dim; ve.seg_dim = d.seg_dim;
    ve.prop_enc = d.prop_enc; ve.seg_enc = d.seg_enc; ve.dtype = (vog_dtype)d.enc_dtype;
    const bool will_pair = pairs_possible && lstm.persistent;     // (the encoders' partner is a persistent BiLSTM layer)
    // lean form (64-row x 128-column workgroups, every fp32 row read once per column half): when the
    // encoders share the launch of a BiLSTM layer (busy-CU time matters, latency is hidden), and for
    // the p100 shapes where the wide form's 8 column slices per row tile re-stream the features
    ve.lean = c->enc_lean < 0 ? ((will_pair || g.rows_obj >= 4096) ? 1 : 0) : c->enc_lean;
    if (c->tx_split) {     // hi + lo operands: the stream form carries them (visenc_dev.h)
      ve.lean = 1;
      ve.w_prop_f_lo = c->w_prop_f_lo; ve.w_seg_f_lo = c->w_seg_f_lo; ve.c16_lo = ws.at<void>("prop_seg16_lo");
    }
    // many proposals per frame: the replication of the segment rows is its own (chip-wide) copy launch,
    // so the encoder kernel stays one launch and can still share the BiLSTM layer's
    const bool rep_step = ve.lean && d.nppf0 > 16 && (d.seg_enc % 4) == 0 && (d.prop_enc % 4) == 0 && (g.d_obj % 4) == 0;
    ve.defer_replicas = rep_step ? 1 : 0;
    vis("vis_enc", [ve](hipStream_t st) { return vog_vis_encode(&ve, st); });
    if (rep_step) vis("seg_rep", [ve](hipStream_t st) { return vog_seg_replicate(&ve, st); });
  }

  // the two encoders as GEMM launches on the 16-bit copies of the features
  void gemm_encoder_steps() {
    float* ps32 = ws.at<float>("prop_seg");
    void* ps16 = ws.at<void>("prop_seg16");
    // the two encoders have 52 / 12 output tiles and K = 2048 / 3072: split K so every CU
    // gets a slice, partial products go to fp32 slabs, one finishing pass for both
    auto pick_split = [](int M, int N, int K) {
      const int64_t tiles = (int64_t)ceil_div(M, 64) * ceil_div(N, 64);
      int sp = (int)((511 + tiles) / tiles);
      const int nk = K / 64;
      if (sp > nk / 4) sp = nk / 4;
      if (sp > 16) sp = 16;
      return sp < 1 ? 1 : sp;
    };
    const int Mp = (int)g.rows_obj, Ms = g.n_vid * g.Fv;
    const bool can_split = (d.prop_dim % 64) == 0 && (d.seg_dim % 64) == 0 && Mp > 64 && Ms > 64 &&
                           (d.prop_enc % 4) == 0 && (d.seg_enc % 4) == 0;
    const int sp_p = can_split ? pick_split(Mp, d.prop_enc, d.prop_dim) : 1;
    const int sp_s = can_split ? pick_split(Ms, d.seg_enc, d.seg_dim) : 1;
    float* slab_p = ws.at<float>("enc_slabs");
    float* slab_s = slab_p + (int64_t)16 * Mp * d.prop_enc;
    vog_gemm_args pe{}; pe.c16_dtype = d.tx_dtype;
    pe.a = ws.at<void>("prop16"); pe.a_is_f32 = 0; pe.lda = d.prop_dim; pe.w = c->w_prop; pe.ldw = d.prop_dim;
    pe.M = Mp; pe.N = d.prop_enc; pe.K = d.prop_dim; pe.rep = 1; pe.dtype = (vog_dtype)d.enc_dtype;
    vog_gemm_args se{}; se.c16_dtype = d.tx_dtype;
    se.a = ws.at<void>("seg16"); se.a_is_f32 = 0; se.lda = d.seg_dim; se.w = c->w_seg; se.ldw = d.seg_dim;
    se.M = Ms; se.N = d.seg_enc; se.K = d.seg_dim; se.dtype = (vog_dtype)d.enc_dtype;
    if (can_split && sp_p > 1 && sp_s > 1) {
      pe.c32 = slab_p; pe.ldc = d.prop_enc; pe.splitk = sp_p;
      se.c32 = slab_s; se.ldc = d.seg_enc; se.splitk = sp_s; se.rep = 1;
      vis("prop_enc", [pe](hipStream_t st) { return vog_gemm_bias_act(&pe, st); });
      vis("seg_enc", [se](hipStream_t st) { return vog_gemm_bias_act(&se, st); });
      vog_splitk_prob f0{}, f1{};
      f0.slabs = slab_p; f0.splits = sp_p; f0.M = Mp; f0.N = d.prop_enc; f0.bias = c->b_prop; f0.relu = 1; f0.rep = 1;
      f0.c32 = ps32; f0.c16 = ps16; f0.ldc = g.d_obj; f0.ldc16 = g.d_obj; f0.c16_dtype = d.tx_dtype;
      f1.slabs = slab_s; f1.splits = sp_s; f1.M = Ms; f1.N = d.seg_enc; f1.bias = c->b_seg; f1.relu = 1; f1.rep = d.nppf0;
      f1.c32 = ps32 + d.prop_enc; f1.c16 = (unsigned short*)ps16 + d.prop_enc; f1.ldc = g.d_obj; f1.ldc16 = g.d_obj;
      f1.c16_dtype = d.tx_dtype;
      vis("enc_finish", [f0, f1](hipStream_t st) { return vog_splitk_finish(&f0, &f1, st); });
    } else {
      pe.bias = c->b_prop; pe.relu = 1; pe.c32 = ps32; pe.c16 = ps16; pe.ldc = g.d_obj; pe.ldc16 = g.d_obj;
      vis("prop_enc", [pe](hipStream_t st) { return vog_gemm_bias_act(&pe, st); });
      se.bias = c->b_seg; se.relu = 1; se.c32 = ps32 + d.prop_enc;
      se.c16 = (unsigned short*)ps16 + d.prop_enc; se.ldc = g.d_obj; se.ldc16 = g.d_obj; se.rep = d.nppf0;
      vis("seg_enc", [se](hipStream_t st) { return vog_gemm_bias_act(&se, st); });
    }
  }

  // prop_seg in its three forms from encoder outputs that came with the batch (vog_vis_concat)
  void concat_step() {
    vog_visconcat_args vc{};
    vc.enc_prop = b->enc_prop; vc.enc_seg = b->enc_seg;
    vc.c32 = ws.at<float>("prop_seg"); vc.c16 = ws.at<void>("prop_seg16");
    vc.c16_lo = c->tx_split ? ws.at<void>("prop_seg16_lo") : nullptr;
    vc.ldc = g.d_obj; vc.c16_dtype = d.tx_dtype;
    vc.n_rows = (int)g.rows_obj; vc.nppf0 = d.nppf0; vc.prop_enc = d.prop_enc; vc.seg_enc = d.seg_enc;
    vis("vis_concat", [vc](hipStream_t st) { return vog_vis_concat(&vc, st); });
  }

  // The 16-bit buffers the LAST obj_tx layer writes (layers alternate between the A and the B set), and which of them it
  // writes at all: the copy typed for mul_tx (none without mul_tx), its remainder on the hi + lo plan
  void obj_last16(void** o16, void** o16_lo) {
    const bool toA = ((c->obj.n_layers - 1) % 2) == 0;
    *o16 = has_mul(d) ? ws.at<void>(toA ? "obj_outA16" : "obj_outB16") : nullptr;
    *o16_lo = (has_mul(d) && c->tx_split) ? ws.at<void>(toA ? "obj_outA16_lo" : "obj_outB16_lo") : nullptr;
  }

  // what the stages behind obj_tx read and the cached rows do not hold (vog_obj_restore)
  void restore_step() {
    vog_objrestore_args ra{};
    ra.x = b->obj_out; ra.ldc = g.d_obj; ra.y16_dtype = d.tx_dtype;
    obj_last16(&ra.y16, &ra.y16_lo);
    if (g.sep) { ra.enc_seg = b->enc_seg; ra.prop_seg = ws.at<float>("prop_seg"); }      // (the sep head: pred_cmp)
    ra.n_rows = (int)g.rows_obj; ra.nppf0 = d.nppf0; ra.d_obj = g.d_obj; ra.seg_enc = d.seg_enc;
    vis("obj_restore", [ra](hipStream_t st) { return vog_obj_restore(&ra, st); });
  }

  // the encoders proper: what vog_ctx_encode_videos runs for a bank of encoded rows, and every forward from raw features
  int raw_encoder_steps() {
    if (enc_fused) fused_encoder_steps();
    else gemm_encoder_steps();
    if (c->tx_split && !(c->fused_enc && c->w_prop_f_lo))
      VOG_FAIL(-5, "tx_split needs the fused feature encoders (feature dims %% 256, encode sizes %% 32 and <= 256)");
    return 0;
  }

  int encoder_steps() {
    if (!fuse_prep) {       // (encoded / cached_obj: the box-bias precursors only, no feature cast)
      const vog_visprep_args vp = visprep_args();
      vis("vis_prep", [vp](hipStream_t st) { return vog_vis_prep(&vp, st); });
    }
    if (cached_obj) { restore_step(); return 0; }
    if (encoded) { concat_step(); return 0; }
    return raw_encoder_steps();
  }

  // QKV projection + attention of one layer, plain and structured
  int tx_attn_steps(const TxStackIO& io, const TxLayerIO& t) {
    const TxWeights& tw = t.tw; const TxLayer& L = t.L;
    const std::string& n = t.n;
    const bool split = c->tx_split != 0;
    const int l = t.l;
    constexpr int kLogitGroup = VOG_LOGIT_WORDS * VOG_LOGIT_STRIDE;                // words of one layer's report
    vog_qkv_args qa{};
    qa.x16 = t.cur16; qa.ldx = tw.d; qa.wqkv = L.wqkv; qa.ldw = tw.d;
    qa.q = ws.at<void>(n + "_q"); qa.k = ws.at<void>(n + "_k"); qa.vt = ws.at<void>(n + "_vt");
    qa.S = io.S; qa.N = io.N; qa.H = tw.H; qa.dp = tw.dp; qa.npad = io.npad; qa.K = tw.d; qa.dtype = t.dt;
    // many rows (p100): one workgroup per 64 rows walks all output columns (qkvrb_dev.h: +1.5 % at cfg 4); the tiled LDS-DMA GEMM
    // otherwise (a 64-row x 512-column row-block form measured -3 % at cfg 2 and was removed in round 6)
    const bool qkv_rb = g.rows_obj >= 8192;
    qa.wqkv_p32 = qkv_rb ? L.wqkv_p : nullptr;
    if (split) {
      qa.x16_lo = t.cur16_lo; qa.wqkv_lo = L.wqkv_lo; qa.q_lo = ws.at<void>(n + "_q_lo"); qa.k_lo = ws.at<void>(n + "_k_lo");
      qa.wqkv_p32 = nullptr;
      if (!qa.x16_lo || !qa.wqkv_lo) VOG_FAIL(-1, "hi + lo operands: layer %d of %s has no remainder rows", l, n.c_str());
    }
    if (t.fact) {
      // layer 0 of mul_tx: tokens are [vis[p] || lang[a]] -> project the two parts once each
      const vog_vislang_args sv = *io.structured;
      vog_qkv_args qs = qa;
      qs.x16 = io.vis16; qs.ldx = sv.dv; qs.K = sv.dv;          // visual rows x first d_vis weight columns
      // nothing is fanned out: q, k, v fragments of the nppf VISUAL tokens of every sequence (a plain
      // QKV projection of the visual rows); the separable attention below adds the language parts
      const int npad_kv = (int)round_up64(sv.nppf, 32);
      qs.N = sv.nppf; qs.npad = npad_kv;
      qs.wqkv_p32 = (qkv_rb && !split) ? L.wqkv_pv : nullptr;
      if (split) qs.x16_lo = io.vis16_lo;
      vis(n + "_pv", [qs](hipStream_t st) { return vog_qkv_proj(&qs, st); });
      vog_attn_struct_args sa{};
      sa.q_visual = 1;
      sa.q = qa.q; sa.kv = qa.k; sa.vv = qa.vt; sa.pl = ws.at<float>(n + "_pl"); sa.out16 = t.attn16;
      sa.u = t.u; sa.pe_b = tw.pe_b; sa.S = io.S; sa.H = tw.H; sa.dp = tw.dp; sa.nsrl = sv.nsrl; sa.nppf = sv.nppf;
      sa.npad_q = io.npad; sa.npad_kv = npad_kv; sa.nfrm = sv.nfrm; sa.lang_per_vid = sv.lang_per_vid;
      sa.nc_v = sv.nc_v; sa.use_rel = tw.use_rel; sa.seq_per_vid = io.seq_per_vid; sa.NP = g.NP;
      sa.inv_scale = 1.0f / sqrtf((float)tw.d); sa.dtype = t.dt;
      sa.guard_flag = (n == "mul") ? ws.at<int>("mul_ef_guard") : nullptr;
      sa.logit_max = t.lmax + (l < 3 ? l : 3) * kLogitGroup;
      if (split) { sa.q_lo = qa.q_lo; sa.kv_lo = qa.k_lo; sa.out16_lo = t.tail_split ? t.attn16_lo : nullptr; }
      vis(n + "_attn", [sa](hipStream_t st) { return vog_rel_attention_struct_fwd(&sa, st); });
      return 0;
    }
    vis(n + "_qkv", [qa](hipStream_t st) { return vog_qkv_proj(&qa, st); });
    vog_attn_args aa{};
    aa.q = qa.q; aa.k = qa.k; aa.vt = qa.vt; aa.out16 = t.attn16;
    aa.u = t.u; aa.pe_b = tw.pe_b; aa.S = io.S; aa.N = io.N; aa.H = tw.H; aa.dp = tw.dp; aa.npad = io.npad;
    aa.use_rel = tw.use_rel; aa.n_box = io.n_box; aa.seq_per_vid = io.seq_per_vid; aa.NP = g.NP;
    aa.inv_scale = 1.0f / sqrtf((float)tw.d); aa.dtype = t.dt;
    // one guard word PER LAYER inside the stack's zero-filled 256 bytes (with one word per stack a flag raised by
    // layer 0 stayed up - the prologue clears once per forward - and every later layer re-ran the running-maximum fallback)
    aa.guard_flag = ws.at<int>(n + "_guard") + (l < 63 ? l : 63);
    aa.guard_precleared = l < 63 ? 1 : 0;
    aa.logit_max = t.lmax + (l < 3 ? l : 3) * kLogitGroup;   // (layers past the 4th share the last group)
    if (split) { aa.q_lo = qa.q_lo; aa.k_lo = qa.k_lo; aa.out16_lo = t.tail_split ? t.attn16_lo : nullptr; }
    vis(n + "_attn", [aa](hipStream_t st) { return vog_rel_attention_fwd(&aa, st); });
    return 0;
  }

  // everything after the attention is row-local: one launch (txtail.hip); with `score` the
  // last layer also runs lin2 + the score head and its output never leaves the chip
  void tx_fused_tail_step(TxStackIO& io, const TxLayerIO& t) {
    const TxWeights& tw = t.tw; const TxLayer& L = t.L;
    vog_tx_tail_args ta{};
    ta.attn16 = t.attn16; ta.kwo = tw.H * tw.dp; ta.wo_p = L.wo_p; ta.w1_p = L.w1_p; ta.w2_p = L.w2_p;
    ta.residual = t.fact ? nullptr : t.cur32; ta.ldr = tw.d;
    ta.ln1g = L.ln1g; ta.ln1b = L.ln1b; ta.b1 = L.b1; ta.b2 = L.b2; ta.ln2g = L.ln2g; ta.ln2b = L.ln2b;
    ta.y32 = t.o32w; ta.y16 = t.o16w; ta.y16_dtype = (int)t.odt;
    ta.x1_scratch = ws.at<float>(t.n + "_x1s");
    ta.M = (int)t.rows; ta.d = tw.d; ta.dh = tw.dh; ta.dtype = t.dt; ta.head_dtype = d.enc_dtype;
    if (t.tail_split) {
      ta.attn16_lo = t.attn16_lo; ta.wo_p_lo = L.wo_p_lo; ta.w1_p_lo = L.w1_p_lo; ta.w2_p_lo = L.w2_p_lo;
      ta.y16_lo = t.o16w ? t.o16_lo : nullptr;
    }
    const bool with_score = t.last && io.score && c->w_lin2_p;
    vog_score_args sc{};
    if (with_score) { sc = *io.score; ta.wl_p = c->w_lin2_p; ta.bl = c->b_lin2; ta.y32 = nullptr; ta.y16 = nullptr; }
    vog_vislang_args sv{};
    const bool fact = t.fact;
    if (fact) sv = *io.structured;
    vis(t.n + "_tail", [ta, fact, sv, with_score, sc](hipStream_t st) {
      vog_tx_tail_args t2 = ta;
      if (fact) t2.res_vislang = &sv;
      if (with_score) t2.score = &sc;
      return vog_tx_tail_fwd(&t2, st); });
    io.score_done = with_score;
  }

  // the same as separate launches: Wo (+ residual), LayerNorm, the two feed-forward GEMMs, LayerNorm
  void tx_unfused_tail_steps(const TxStackIO& io, const TxLayerIO& t) {
    const TxWeights& tw = t.tw; const TxLayer& L = t.L;
    const std::string& n = t.n;
    const vog_dtype dt = t.dt, odt = t.odt;
    const int rows = (int)t.rows, d_ = tw.d;
    vog_gemm_args wo{}; wo.c16_dtype = -1;
    wo.a = t.attn16; wo.a_is_f32 = 0; wo.lda = (int64_t)tw.H * tw.dp; wo.w = L.wo; wo.ldw = (int64_t)tw.H * tw.dp;
    wo.residual = t.cur32; wo.ldr = tw.d; wo.c32 = ws.at<float>(n + "_tmp"); wo.ldc = tw.d;
    wo.M = rows; wo.N = tw.d; wo.K = tw.H * tw.dp; wo.rep = 1; wo.dtype = dt;
    if (t.fact) {
      const vog_vislang_args sv = *io.structured;       // residual = the (unmaterialised) token matrix
      wo.residual = nullptr;
      vis(n + "_wo", [wo, sv](hipStream_t st) {
        vog_gemm_args w2 = wo; w2.res_vislang = &sv; return vog_gemm_bias_act(&w2, st); });
    } else {
      vis(n + "_wo", [wo](hipStream_t st) { return vog_gemm_bias_act(&wo, st); });
    }
    float *x1 = ws.at<float>(n + "_x1"), *tmp = wo.c32;
    void* x1_16 = ws.at<void>(n + "_x1_16");
    const float *ln1g = L.ln1g, *ln1b = L.ln1b, *ln2g = L.ln2g, *ln2b = L.ln2b;
    vis(n + "_ln1", [tmp, ln1g, ln1b, x1, x1_16, rows, d_, dt](hipStream_t st) {
      return vog_residual_layernorm(tmp, ln1g, ln1b, x1, x1_16, rows, d_, dt, st); });
    vog_gemm_args f1{}; f1.c16_dtype = -1;
    f1.a = x1_16; f1.lda = tw.d; f1.w = L.w1; f1.ldw = tw.d; f1.bias = L.b1; f1.relu = 1;
    f1.c16 = ws.at<void>(n + "_ffn16"); f1.ldc16 = tw.dh; f1.M = rows; f1.N = tw.dh; f1.K = tw.d;
    f1.rep = 1; f1.dtype = dt;
    vis(n + "_ffn1", [f1](hipStream_t st) { return vog_gemm_bias_act(&f1, st); });
    vog_gemm_args f2{}; f2.c16_dtype = -1;
    f2.a = f1.c16; f2.lda = tw.dh; f2.w = L.w2; f2.ldw = tw.dh; f2.bias = L.b2; f2.residual = x1;
    f2.ldr = tw.d; f2.c32 = tmp; f2.ldc = tw.d; f2.M = rows; f2.N = tw.d; f2.K = tw.dh; f2.rep = 1;
    f2.dtype = dt;
    vis(n + "_ffn2", [f2](hipStream_t st) { return vog_gemm_bias_act(&f2, st); });
    float* o32w = t.o32w; void* o16w = t.o16w;
    vis(n + "_ln2", [tmp, ln2g, ln2b, o32w, o16w, rows, d_, odt](hipStream_t st) {
      return vog_residual_layernorm(tmp, ln2g, ln2b, o32w, o16w, rows, d_, odt, st); });
  }

  int tx_stack_steps(const TxWeights& tw, const char* nm, TxStackIO& io) {
    const std::string n(nm);
    const vog_dtype dt = (vog_dtype)d.tx_dtype;
    const bool split = c->tx_split != 0;
    constexpr int kLogitGroup = VOG_LOGIT_WORDS * VOG_LOGIT_STRIDE;
    unsigned int* lmax = ws.at<unsigned int>("logit_max") + (n == "mul" ? 4 * kLogitGroup : 0);
    // (the bias precursors u are produced by the fused visual prologue)
    float* u = ws.at<float>(n + "_u");
    io.out32 = io.x32; io.out16 = io.x16; io.out16_lo = io.x16_lo; io.score_done = false;
    for (int l = 0; l < tw.n_layers; ++l) {
      const bool toA = (l % 2) == 0, last = l == tw.n_layers - 1;
      TxLayerIO t{tw, tw.layers[l], n, l, dt, (int64_t)io.S * io.N};
      t.fact = io.structured && l == 0; t.last = last;
      t.tail_split = split && (!last || io.out_feeds_attn);
      t.cur32 = io.out32; t.cur16 = io.out16; t.cur16_lo = io.out16_lo;
      t.u = u; t.lmax = lmax;
      t.attn16 = ws.at<void>(n + "_attn16");
      t.attn16_lo = split ? ws.at<void>(n + "_attn16_lo") : nullptr;
      t.o32 = ws.at<float>(n + (toA ? "_outA" : "_outB"));
      t.o16 = ws.at<void>(n + (toA ? "_outA16" : "_outB16"));
      t.o16_lo = split ? ws.at<void>(n + (toA ? "_outA16_lo" : "_outB16_lo")) : nullptr;
      // 16-bit copy of the LAST layer's output: typed for its consumer (none for obj_tx,
      // the f16 score head for mul_tx)
      t.o16w = (last && io.last_dt < 0) ? nullptr : t.o16;
      t.odt = last && io.last_dt >= 0 ? (vog_dtype)io.last_dt : dt;
      // the last layer's fp32 output is written only if somebody reads it (mul_tx: the score
      // head takes the 16-bit copy -> 12 MB less HBM traffic per forward at cfg 2)
      t.o32w = (last && !io.last_needs_f32 && t.o16w) ? nullptr : t.o32;
      VOG_TRY(tx_attn_steps(io, t));
      const bool fused = c->fused_tail && t.L.wo_p && tx_tail_supported(tw.d, tw.dh, tw.H * tw.dp);
      if (fused && (!split || tx_tail_split_supported(tw.d, tw.dh, tw.H * tw.dp))) {
        tx_fused_tail_step(io, t);
        io.out16_lo = t.tail_split ? t.o16_lo : nullptr;
      } else {
        if (split) VOG_FAIL(-1, "hi + lo operands need the fused encoder-layer tail (d = 512 / 768; stack %s)", nm);
        tx_unfused_tail_steps(io, t);
      }
      io.out32 = t.o32; io.out16 = t.o16;
    }
    return 0;
  }

  // obj_tx over prop_seg (a7, a8): what build_steps and vog_ctx_obj_videos hand to tx_stack_steps
  TxStackIO obj_stack_io() {
    TxStackIO obj{};
    obj.x32 = ws.at<float>("prop_seg"); obj.x16 = ws.at<void>("prop_seg16");
    obj.x16_lo = c->tx_split ? ws.at<void>("prop_seg16_lo") : nullptr;
    obj.S = g.S_obj; obj.N = g.N_obj; obj.npad = g.npad_obj; obj.seq_per_vid = g.spv_obj; obj.n_box = g.N_obj;
    obj.last_dt = has_mul(d) ? d.tx_dtype : -1; obj.last_needs_f32 = true; obj.out_feeds_attn = has_mul(d);
    return obj;
  }

  // ---- vis || lang tokens in mul_tx order (a10, a11) --------------------------------------------------------
  vog_vislang_args vislang_args(const float* vis32) {
    vog_vislang_args va{};
    va.vis = vis32; va.lang = lang_vec; va.x32 = ws.at<float>("xmul"); va.x16 = ws.at<void>("xmul16");
    va.n_vid = g.n_vid; va.nfrm = g.nfrm; va.nppf = g.nppf; va.nsrl = d.nsrl; va.dv = g.d_obj; va.dl = g.L;
    va.lang_per_vid = g.nvl > 1 ? 1 : 0; va.nc_v = g.nc_v; va.dtype = (vog_dtype)(has_mul(d) ? d.tx_dtype : d.enc_dtype);
    return va;
  }

  vog_score_args score_args() {
    vog_score_args sa{};
    sa.w2 = c->w_lin2b; sa.b2 = c->b_lin2b; sa.arg_msk = b->srl_arg_inds_msk;
    sa.cmp_msk = b->num_cmp_msk; sa.outs = b->mdl_outs; sa.outs_eval = b->mdl_outs_eval;
    sa.n_vid = g.n_vid; sa.nfrm = g.nfrm; sa.nppf = g.nppf; sa.nsrl = d.nsrl; sa.dh = 256;
    sa.conc_type = d.conc_type; sa.ncmp = g.ncmp; sa.nc_v = g.nc_v; sa.nvl = g.nvl;
    sa.nfrm0 = d.nfrm0; sa.nppf0 = d.nppf0;
    return sa;
  }

  // ---- heads (a9 tail / a20 / a17); x16: the 16-bit rows lin2 reads; score_done: the fused mul_tx tail already ran lin2 + score
  void head_steps(vog_score_args sa, const void* x16, bool score_done) {
    if (!score_done) {
      vog_gemm_args l2{}; l2.c16_dtype = -1;
      l2.a = x16; l2.a_is_f32 = 0;               // (the 16-bit copy feeding lin2 is always written in the head's type)
      l2.lda = g.d_mul; l2.w = c->w_lin2; l2.ldw = g.d_mul; l2.bias = c->b_lin2; l2.relu = 1;
      l2.c32 = ws.at<float>("h1"); l2.ldc = 256; l2.M = (int)g.rows_mul; l2.N = 256; l2.K = g.d_mul;
      l2.rep = 1; l2.dtype = (vog_dtype)d.enc_dtype;
      vis("lin2", [l2](hipStream_t st) { return vog_gemm_bias_act(&l2, st); });
      sa.h1 = l2.c32;
      vis("score", [sa](hipStream_t st) { return vog_score_head(&sa, st); });
    }
    if (g.sep) {
      vog_predcmp_args pa{};
      pa.final_hidden = shared ? b->shared_final_hidden : ws.at<float>("full") + (int64_t)g.Bn * g.T * g.L;
      pa.prop_seg = ws.at<float>("prop_seg"); pa.w0 = c->w_sv0; pa.b0 = c->b_sv0; pa.w2 = c->w_sv2; pa.b2 = c->b_sv2;
      pa.outs = b->mdl_outs; pa.arg_msk = b->srl_arg_inds_msk; pa.cmp_msk = b->num_cmp_msk;
      pa.verb_ind = b->verb_ind_in_srl; pa.vidf_outs = b->vidf_outs; pa.fin_scores_loss = b->fin_scores_loss;
      pa.fin_scores = b->fin_scores; pa.B = g.B; pa.ncmp = g.ncmp; pa.nvl = g.nvl; pa.nsrl = d.nsrl;
      pa.NP = g.NP; pa.nfrm0 = d.nfrm0; pa.nppf0 = d.nppf0; pa.L = g.L; pa.dp0 = d.prop_enc; pa.dps = g.d_obj;
      vis("pred_cmp", [pa](hipStream_t st) { return vog_pred_cmp_head(&pa, st); });
    }
    if (b->pred_rec) {
      vog_pred_args pr{};
      pr.outs_eval = b->mdl_outs_eval; pr.props = b->pad_proposals; pr.fin_scores = b->fin_scores;
      pr.rec = b->pred_rec; pr.B = g.B; pr.ncmp = g.ncmp; pr.nsrl = d.nsrl; pr.nfrm0 = d.nfrm0;
      pr.nppf0 = d.nppf0; pr.conc_type = d.conc_type;
      pr.logit_max = ws.at<unsigned int>("logit_max"); pr.stats = b->stats; pr.published = ws.at<unsigned int>("logit_pub");
      vis("pred_head", [pr](hipStream_t st) { return vog_pred_head(&pr, st); });
    }
  }

  // ---- horizontal fusion (pair.hip): the language chain and the visual chain are independent until
  // mul_tx's attention, and neither fills the chip (the persistent BiLSTM layer holds 64 CUs for
  // ~46 us): step i of one shares a launch with step i of the other. The visual step moves up to the
  // language step's position (its own inputs are produced by earlier pairs); combinations without a
  // registered pair kernel fall back to two launches inside pair_launch.
  // A batch with argument vectors AND banked visual rows starts with mul_pl, vis_prep (box-bias precursors only) and vis_concat /
  // obj_restore: three small launches that read batch inputs and weights only and write disjoint buffers (mul_pl; obj_u / mul_u;
  // prop_seg and the 16-bit row copies). They become ONE launch, bank_prep (elementwise.hip), where the fused kernel carries their
  // forms: structured mul_tx layer 0, M <= 64 rows with fragment-ordered weights, lang_enc <= 256 (the short-K body), 16-byte
  // aligned rows (the 8-column form of the row copy), "pair_launches" on. The hi + lo plan keeps the three launches (its mul_pl
  // is up to several launches of the split body), and so does everything else.
  void bank_prep_pass() {
    if (!bank_fuse || steps.size() < 3) return;
    const char* rows = cached_obj ? "obj_restore" : "vis_concat";
    if (steps[0].name != "mul_pl" || steps[1].name != "vis_prep" || steps[2].name != rows) return;
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (g.Bn * d.nsrl > 64 || !c->mul.layers[0].wqkv_lang_f || g.L > 256) return;
    if (!a16(b->enc_seg) || !a16(cached_obj ? b->obj_out : b->enc_prop) || !a16(b->shared_lang)) return;
    auto fg = steps[0].fn, fp = steps[1].fn, fr = steps[2].fn;
    Step m{"bank_prep", [fg, fp, fr](hipStream_t st) { return bank_prep_launch(fg, fp, fr, st); }, Chain::Prologue};
    steps.erase(steps.begin(), steps.begin() + 3);
    steps.insert(steps.begin(), m);
  }

  void pair_pass() {
    if (!pairs_possible) return;
    auto find = [&](const char* nm, int occurrence) {
      for (size_t i = 0; i < steps.size(); ++i)
        if (steps[i].name == nm && occurrence-- == 0) return (int)i;
      return -1;
    };
    // language step -> visual step that shares its launch (+ a visual step that follows on its own).
    // Pairs are chosen by shape: a 512-thread body next to a 512-thread body, 256 next to 256 (a
    // register-heavy 512-thread partner would cut the occupancy of a small-block streaming kernel:
    // input projection + encoders in one grid measured 29.8 us against 6.4 + 16.0 apart).
    // The BiLSTM layers (64 CUs for ~38 us each) take the encoders and the obj_tx tail as partners; the
    // obj_tx QKV projection and attention follow the first pair on their own (paired with the layer-1
    // input projection they measured SLOWER than apart: 22.5 vs 9.5 + 7.4 us).
    // alone: the language step keeps its launch and the visual steps only move up behind it (encoded inputs: vis_concat is a
    // microsecond copy, no partner for a BiLSTM layer - but obj_tx's QKV projection and attention must still run before layer
    // 1's launch, which carries the obj_tx tail)
    struct Want { const char* lang; int occ; const char* vis; const char* then[3]; bool alone; };
    const bool has_rep = find("seg_rep", 0) >= 0;
    // where layer 1's input projection is a GEMM launch (more than 80 columns) obj_tx's QKV projection shares THAT launch
    // (pair_mask bit 8) and the attention follows it, instead of both following the first pair on their own
    // Measured (scratch/r6_ae.sh, three interleaved runs each): cfg 3 (Bn x T = 96: the projection is 256 tiles, one per CU) 68.2 vs
    // 66.9 k queries/s; cfg 5 (192 columns: 384 tiles) 111.5 vs 113.1 k - the pair only where the projection leaves room on the chip.
    const bool ih1_pair = find("lstm_ih1", 0) >= 0 && find("obj_qkv", 0) >= 0 && ((c->pair_mask >> 3) & 1) && g.Bn * g.T <= 128;
    std::vector<Want> want;
    if (cached_obj) {       // (obj_restore is a microsecond copy as well; there is no obj_tx step left to place)
      want.push_back(Want{"lstm_layer", 0, "obj_restore", {nullptr, nullptr, nullptr}, true});
    } else if (encoded) {
      want.push_back(ih1_pair ? Want{"lstm_layer", 0, "vis_concat", {nullptr, nullptr, nullptr}, true}
                              : Want{"lstm_layer", 0, "vis_concat", {"obj_qkv", "obj_attn", nullptr}, true});
    } else if (!ih1_pair) {
      want.push_back(has_rep ? Want{"lstm_layer", 0, "vis_enc", {"seg_rep", "obj_qkv", "obj_attn"}}
                             : Want{"lstm_layer", 0, "vis_enc", {"obj_qkv", "obj_attn", nullptr}});
    } else {
      want.push_back(has_rep ? Want{"lstm_layer", 0, "vis_enc", {"seg_rep", nullptr, nullptr}}
                             : Want{"lstm_layer", 0, "vis_enc", {nullptr, nullptr, nullptr}});
    }
    if (!cached_obj) want.push_back({"lstm_layer", 1, "obj_tail", {nullptr, nullptr, nullptr}});      // (cached: layer 1 runs alone)
    want.push_back({"lstm_outproj", 0, "mul_pv", {nullptr, nullptr, nullptr}});
    if (ih1_pair) want.insert(want.begin() + 1, Want{"lstm_ih1", 0, "obj_qkv", {"obj_attn", nullptr, nullptr}});
    struct Plan2 { int ia, ib; int it[3]; bool alone; };
    std::vector<Plan2> plans;
    bool ok = true;
    int prev_vis = -1;
    for (auto& w : want) {
      const int bit = std::string(w.lang) == "lstm_ih1" ? 3 : (std::string(w.lang) == "lstm_outproj" ? 2 : w.occ);
      if (!((c->pair_mask >> bit) & 1)) continue;      // this pair stays two launches (its visual step keeps its place)
      Plan2 q{find(w.lang, w.occ), find(w.vis, 0), {-1, -1, -1}, w.alone};
      // every visual step only moves EARLIER (its producers sit in earlier pairs) and the visual chain
      // keeps its own order; any missing piece (other model variants / shapes) leaves the rest unpaired
      if (q.ia < 0 || q.ib < 0 || q.ib < q.ia || q.ib < prev_vis) { ok = false; break; }
      int last = q.ib;
      for (int k = 0; k < 3 && w.then[k]; ++k) {
        q.it[k] = find(w.then[k], 0);
        if (q.it[k] < last) { ok = false; break; }
        last = q.it[k];
      }
      if (!ok) break;
      prev_vis = last;
      plans.push_back(q);
    }
    if (plans.empty()) ok = false;
    if (ok) {
      // nothing else of the visual chain may sit between the moved steps (it would be overtaken)
      std::vector<int> moved;
      for (auto& q : plans) { moved.push_back(q.ib); for (int k = 0; k < 3; ++k) if (q.it[k] >= 0) moved.push_back(q.it[k]); }
      for (int i = moved.front(); i <= moved.back() && ok; ++i)
        if (steps[i].chain == Chain::Visual && std::find(moved.begin(), moved.end(), i) == moved.end()) ok = false;
    }
    if (!ok) return;
    std::vector<int> role(steps.size(), 0);           // 1 = removed from its old position
    std::vector<Step> out;
    for (auto& q : plans) { role[q.ib] = 1; for (int k = 0; k < 3; ++k) if (q.it[k] >= 0) role[q.it[k]] = 1; }
    for (size_t i = 0; i < steps.size(); ++i) {
      if (role[i]) continue;
      const Plan2* q = nullptr;
      for (auto& x : plans) if (x.ia == (int)i) q = &x;
      if (!q) { out.push_back(steps[i]); continue; }
      Step m = steps[i];
      if (q->alone) {
        out.push_back(m);
        Step v = steps[q->ib]; v.chain = m.chain; out.push_back(v);
      } else {
        auto fa = steps[q->ia].fn, fb = steps[q->ib].fn;
        m.name = steps[q->ia].name + "+" + steps[q->ib].name;
        m.fn = [fa, fb](hipStream_t st) { return pair_launch(fa, fb, st, nullptr); };
        out.push_back(m);
      }
      for (int k = 0; k < 3; ++k)
        if (q->it[k] >= 0) { Step t = steps[q->it[k]]; t.chain = m.chain; out.push_back(t); }
    }
    steps.swap(out);
  }

};

// lang_only: only the language inputs of `b` are read. b->shared_lang != NULL: argument vectors (and the final hidden states
// for the sep head) come from a group encoder's workspace.
static int check_batch(const vog_ctx* c, const vog_batch* b, size_t ws_bytes, bool lang_only, Geo& g, Plan& plan) {
  const vog_model_desc& d = c->d;
  VOG_CHECK_ARG(b);
  if (!lang_only) {       // (pure pointer checks first: they need no device, and they name what is wrong)
    if (b->obj_out) {
      if (!b->enc_seg) VOG_FAIL(-1, "vog_batch: obj_out comes with enc_seg (the sep head reads the segment encodings)");
      if (b->enc_prop || b->pad_region_feature || b->seg_feature_for_frms)
        VOG_FAIL(-1, "vog_batch: obj_out stands in place of enc_prop and of the raw features (pad_region_feature / "
                     "seg_feature_for_frms), not next to them");
      if (d.conc_type != VOG_CONC_SEP || !has_obj(d))
        VOG_FAIL(-1, "vog_batch: obj_out needs a sep / svsq model with an object transformer (elsewhere obj_tx attends across "
                     "the videos of a query, or does not exist: an EncodedBank already covers this model)");
    } else if ((b->enc_prop != nullptr) != (b->enc_seg != nullptr))
      VOG_FAIL(-1, "vog_batch: enc_prop and enc_seg come together (both or neither)");
    if (!b->obj_out && !b->enc_prop && !(b->pad_region_feature && b->seg_feature_for_frms))
      VOG_FAIL(-1, "vog_batch: neither raw features (pad_region_feature + seg_feature_for_frms) nor encodings (enc_prop + enc_seg)");
  }
  VOG_CHECK_ARG(c->finalized);
  VOG_CHECK_ARG(b->B > 0 && b->ncmp > 0 && b->T > 0 && b->T <= d.seq_len);
  const bool shared = !lang_only && b->shared_lang != nullptr;
  VOG_CHECK_ARG(b->srl_arg_inds_msk != nullptr);
  VOG_CHECK_ARG(shared || (b->srl_arg_words_ind && b->srl_arg_word_mask && b->srl_arg_word_mask_len &&
                           b->srl_arg_words_capture));
  VOG_CHECK_ARG(lang_only || (b->num_cmp_msk && b->pad_proposals && b->mdl_outs && b->mdl_outs_eval));
  g = make_geo(d, b->B, b->ncmp, b->T);
  VOG_CHECK_ARG(lang_only || !g.sep || (b->verb_ind_in_srl && b->vidf_outs && b->fin_scores && b->fin_scores_loss));
  VOG_CHECK_ARG(!shared || !g.sep || b->shared_final_hidden);
  plan = make_plan(c, g, lang_only);
  if ((int64_t)ws_bytes < plan.total) VOG_FAIL(-2, "workspace too small: %zu < %lld", ws_bytes, (long long)plan.total);
  return 0;
}

// VOG_SKIP_STEPS=name,name,... (perf experiments only; results are WRONG): drop steps whose
// name starts with one of the entries, to measure their marginal cost in the throughput regime
static void skip_filter(std::vector<Step>& steps) {
  const char* skip = perf_env("VOG_SKIP_STEPS");
  if (!skip) return;
  std::vector<std::string> pre;
  std::string cur;
  for (const char* q = skip;; ++q) {
    if (*q == ',' || *q == 0) { if (!cur.empty()) pre.push_back(cur); cur.clear(); if (!*q) break; }
    else cur.push_back(*q);
  }
  std::vector<Step> kept;
  for (auto& s : steps) {
    bool drop = false;
    for (auto& pfx : pre) drop |= s.name.rfind(pfx, 0) == 0;
    if (!drop) kept.push_back(s);
  }
  steps.swap(kept);
}

// The launch sequence of one forward. lang_only: just the language chain of `b` (group encoder, vog_lang_forward) on the
// language-only workspace plan. b->shared_lang != NULL: the language chain is NOT run (a group member).
static int build_steps(const vog_ctx* c, const vog_batch* b, void* wsp, size_t ws_bytes,
                       Plan& plan, std::vector<Step>& steps, bool lang_only = false, bool allow_pairs = true) {
  Geo g;
  VOG_TRY(check_batch(c, b, ws_bytes, lang_only, g, plan));
  Builder B(c, b, g, WS{(char*)wsp, &plan}, steps, lang_only, allow_pairs);
  const vog_model_desc& d = c->d;
  if (!B.shared) VOG_TRY(B.language_steps());
  if (B.structured && !lang_only) VOG_TRY(B.mul_lang_proj_step());
  if (lang_only) return 0;
  VOG_TRY(B.encoder_steps());
  // ---- object transformer (a7, a8)
  TxStackIO obj = B.obj_stack_io();
  if (B.cached_obj) {     // the stack's results came with the batch: fp32 rows in place, 16-bit copies by obj_restore
    void *o16 = nullptr, *o16_lo = nullptr;
    B.obj_last16(&o16, &o16_lo);
    obj.out32 = b->obj_out; obj.out16 = o16; obj.out16_lo = o16_lo;
  } else if (has_obj(d)) VOG_TRY(B.tx_stack_steps(c->obj, "obj", obj));
  else { obj.out32 = obj.x32; obj.out16 = obj.x16; obj.out16_lo = obj.x16_lo; }
  // mul_tx consumes the token structure directly (layer-0 QKV and its residual), so the
  // token matrix is only materialised for ImgGrnd / VidGrnd, whose lin2 reads it
  const vog_vislang_args va = B.vislang_args(obj.out32);
  if (!B.structured) B.vis("vislang", [va](hipStream_t st) { return vog_vislang_layout(&va, st); });
  // ---- multi-modal transformer (a9)
  const vog_score_args sa = B.score_args();
  TxStackIO mul{};
  mul.x32 = va.x32; mul.x16 = va.x16;
  // (not structured: mul_tx would read the materialised token matrix, which has no remainder copy)
  mul.x16_lo = mul.vis16_lo = B.structured ? obj.out16_lo : nullptr;
  mul.vis16 = obj.out16;
  mul.S = g.S_mul; mul.N = g.N_mul; mul.npad = g.npad_mul; mul.seq_per_vid = g.nfrm; mul.n_box = g.nppf;
  mul.last_dt = d.enc_dtype; mul.last_needs_f32 = false; mul.structured = B.structured ? &va : nullptr;
  mul.score = d.enc_dtype == VOG_F16 ? &sa : nullptr;
  mul.out16 = mul.x16;
  if (has_mul(d)) VOG_TRY(B.tx_stack_steps(c->mul, "mul", mul));
  if (c->tx_split && has_mul(d) && !B.structured)
    VOG_FAIL(-5, "tx_split needs the structured mul_tx layer 0 (d_obj %% 64 == 0, lang_enc %% 32 == 0, more than 64 visual rows)");
  B.head_steps(sa, mul.out16, mul.score_done);
  B.bank_prep_pass();
  B.pair_pass();
  skip_filter(steps);
  return 0;
}

}  // namespace vog

// =============================================================================
// C ABI
// =============================================================================
extern "C" int vog_version(void) { return VOG_ABI_VERSION; }
extern "C" const char* vog_last_error(void) { return vog::g_err; }

extern "C" int vog_ctx_create(const vog_model_desc* d, vog_ctx** out) {
  VOG_CHECK_ARG(d && out);
  VOG_CHECK_ARG(d->mdl_kind >= 0 && d->mdl_kind <= 2 && d->conc_type >= 0 && d->conc_type <= 2);
  VOG_CHECK_ARG(d->rnn_size % 32 == 0 && d->emb_dim % 8 == 0 && d->prop_dim % 8 == 0 && d->seg_dim % 8 == 0);
  VOG_CHECK_ARG(d->prop_enc % 8 == 0 && d->seg_enc % 8 == 0 && d->lang_enc % 8 == 0);
  VOG_CHECK_ARG(((d->prop_enc + d->seg_enc) / 2) % 8 == 0 && ((d->prop_enc + d->seg_enc + d->lang_enc) / 2) % 8 == 0);
  VOG_CHECK_ARG(d->nsrl > 0 && d->seq_len > 0 && d->nfrm0 > 0 && d->nppf0 > 0 && d->rnn_layers > 0 && d->rnn_layers <= kMaxRnnLayers);
  vog_ctx* c = new vog_ctx();
  c->d = *d;
  // VOG_LSTM_PERSISTENT=0/1 presets the option (test sweeps); vog_ctx_set_int overrides it
  // HIP streams map onto GPU_MAX_HW_QUEUES hardware queues (default 4 = the co-residency limit of the
  // persistent BiLSTM layer kernel: 4 instances x 64 CUs): with more queues it is off by default
  if (const char* e = getenv("GPU_MAX_HW_QUEUES")) { if (atoi(e) > 4) c->lstm_persistent = 0; }
  if (const char* e = getenv("VOG_LSTM_PERSISTENT")) c->lstm_persistent = atoi(e) ? 1 : 0;
  if (const char* e = perf_env("VOG_FUSED_IH")) c->fused_ih = atoi(e);
  const int R = d->rnn_size, E = d->emb_dim, L = d->lang_enc;
  add_w(c, "lstm_encoder.embed_tokens.weight", (int64_t)(d->vocab_size + 1) * E);
  for (int l = 0; l < d->rnn_layers; ++l)
    for (const char* sfx : {"", "_reverse"}) {
      const int in = l == 0 ? E : 2 * R;
      std::string s = "_l" + std::to_string(l) + sfx;
      add_w(c, "lstm_encoder.lstm.weight_ih" + s, (int64_t)4 * R * in);
      add_w(c, "lstm_encoder.lstm.weight_hh" + s, (int64_t)4 * R * R);
      add_w(c, "lstm_encoder.lstm.bias_ih" + s, 4 * R);
      add_w(c, "lstm_encoder.lstm.bias_hh" + s, 4 * R);
    }
  add_w(c, "lstm_out_feat_proj.0.weight", (int64_t)L * 2 * R);
  add_w(c, "lstm_out_feat_proj.0.bias", L);
  add_w(c, "srl_arg_words_out_enc.0.weight", (int64_t)L * 2 * L);
  add_w(c, "srl_arg_words_out_enc.0.bias", L);
  add_w(c, "prop_encoder.0.weight", (int64_t)d->prop_enc * d->prop_dim);
  add_w(c, "prop_encoder.0.bias", d->prop_enc);
  add_w(c, "seg_encoder.0.weight", (int64_t)d->seg_enc * d->seg_dim);
  add_w(c, "seg_encoder.0.bias", d->seg_enc);
  add_w(c, "seg_verb_classf.0.weight", (int64_t)256 * (d->seg_enc + L));
  add_w(c, "seg_verb_classf.0.bias", 256);
  add_w(c, "seg_verb_classf.2.weight", 256);
  add_w(c, "seg_verb_classf.2.bias", 1);
  const int d_obj = d->prop_enc + d->seg_enc, d_mul = d_obj + L;
  add_w(c, "lin2.0.weight", (int64_t)256 * d_mul);
  add_w(c, "lin2.0.bias", 256);
  add_w(c, "lin2.2.weight", 256);
  add_w(c, "lin2.2.bias", 1);
  if (has_obj_weights(*d)) {
    declare_tx(c, "obj_txf", d_obj, d->obj_layers);
    add_w(c, "pe_obj_sub_enc.0.weight", (int64_t)d->obj_heads * 5);
    add_w(c, "pe_obj_sub_enc.0.bias", d->obj_heads);
  }
  if (has_mul(*d)) {
    declare_tx(c, "mult_txf", d_mul, d->mul_layers);
    add_w(c, "pe_mul_sub_enc.0.weight", (int64_t)d->mul_heads * 5);
    add_w(c, "pe_mul_sub_enc.0.bias", d->mul_heads);
  }
  *out = c;
  return 0;
}

extern "C" int vog_ctx_num_weights(const vog_ctx* c) { return c ? (int)c->names.size() : -1; }
extern "C" const char* vog_ctx_weight_name(const vog_ctx* c, int i) {
  return (c && i >= 0 && i < (int)c->names.size()) ? c->names[i].c_str() : nullptr;
}
extern "C" int64_t vog_ctx_weight_numel(const vog_ctx* c, int i) {
  return (c && i >= 0 && i < (int)c->names.size()) ? c->numel.at(c->names[i]) : -1;
}

// A state-dict key as the context knows it: 0 = `*out` is a declared weight, 1 = a key that is ignored on purpose, < 0 = unknown.
static int normalise_weight_name(const vog_ctx* c, const char* name, std::string* out) {
  std::string n(name);
  if (n.rfind("module.", 0) == 0) n = n.substr(7);          // DDP-wrapped checkpoints (trn_utils.py:536-592)
  // transformers trained with mdl.{obj,mul}_tx.use_ddp=True keep an inner `module.` (mdl_vog.py:441-445,577-578)
  for (const char* pre : {"mult_txf.", "obj_txf."}) {
    const std::string pm = std::string(pre) + "module.";
    if (n.rfind(pm, 0) == 0) n = std::string(pre) + n.substr(pm.size());
  }
  // legacy LayerNorm parameter names (trn_utils.py:560-565)
  for (const char* pr : {".gamma", ".beta"}) {
    const std::string suf(pr);
    if (n.size() > suf.size() && n.compare(n.size() - suf.size(), suf.size(), suf) == 0 &&
        n.find("layernorm") != std::string::npos)
      n = n.substr(0, n.size() - suf.size()) + (suf == ".gamma" ? ".weight" : ".bias");
  }
  if (!c->numel.count(n)) {
    // parameters that exist in reference checkpoints but are not read by forward: srl_simple_lin and
    // lin_tmp always; a transformer's weights only when THIS model variant does not declare that
    // transformer at all (a VidGrnd / VOGNet checkpoint loaded into a smaller variant). A key of a
    // declared transformer that does not match is an error, never silently dropped.
    const bool obj_decl = has_obj_weights(c->d), mul_decl = has_mul(c->d);
    if (n.rfind("srl_simple_lin", 0) == 0 || n.rfind("lin_tmp", 0) == 0 ||
        (!obj_decl && (n.rfind("obj_txf", 0) == 0 || n.rfind("pe_obj_sub_enc", 0) == 0)) ||
        (!mul_decl && (n.rfind("mult_txf", 0) == 0 || n.rfind("pe_mul_sub_enc", 0) == 0)))
      return 1;
    VOG_FAIL(-3, "unexpected weight '%s'", name);
  }
  *out = n;
  return 0;
}

extern "C" int vog_ctx_set_weight(vog_ctx* c, const char* name, const float* host, int64_t numel) {
  VOG_CHECK_ARG(c && name && host);
  std::string n;
  const int nrc = normalise_weight_name(c, name, &n);
  if (nrc != 0) return nrc < 0 ? nrc : 0;
  const int64_t want = c->numel.at(n);
  if (want != numel) VOG_FAIL(-3, "weight '%s': numel %lld, expected %lld", name, (long long)numel, (long long)want);
  c->host[n].assign(host, host + numel);
  c->stale.erase(n);
  c->finalized = false;
  return 0;
}

// ---- image table, device refresh --------------------------------------------------------------------------------
extern "C" int vog_ctx_num_images(const vog_ctx* c) { return (c && c->finalized) ? (int)c->images.size() : -1; }

extern "C" int vog_ctx_image_info(const vog_ctx* c, int i, vog_image_info* out) {
  VOG_CHECK_ARG(c && out && c->finalized && i >= 0 && i < (int)c->images.size());
  const WImage& m = c->images[i];
  memset(out, 0, sizeof(*out));
  out->name = m.name.c_str(); out->dev = m.g.dst; out->bytes = m.g.bytes;
  out->kind = m.kind; out->dtype = m.g.dt; out->lo = m.g.lo;
  out->n_src = (int)m.srcs.size();
  for (int s = 0; s < out->n_src && s < VOG_IMAGE_MAX_SRC; ++s) out->src[s] = m.srcs[s].c_str();
  return 0;
}

// Rewrite the weight images of a finalized context in place from fp32 device tensors (wpack.hip): same addresses, same bytes
// as vog_ctx_finalize would make from the same values. Everything is checked before the first launch; after the first call
// on a context nothing is allocated, and the host never waits for the device here.
extern "C" int vog_ctx_refresh_device(vog_ctx* c, const vog_weight_src* srcs, int n, void* stream) {
  VOG_CHECK_ARG(c && (srcs || n == 0) && n >= 0);
  if (!c->finalized) VOG_FAIL(-2, "vog_ctx_refresh_device: the context is not finalized (vog_ctx_finalize builds the images first)");
  hipStream_t st = (hipStream_t)stream;
  std::map<std::string, const float*> given;
  for (int i = 0; i < n; ++i) {
    VOG_CHECK_ARG(srcs[i].name);
    std::string nm;
    const int nrc = normalise_weight_name(c, srcs[i].name, &nm);
    if (nrc < 0) return nrc;
    if (nrc == 1) continue;
    if (!srcs[i].dev) VOG_FAIL(-3, "weight '%s': NULL device pointer", srcs[i].name);
    const int64_t want = c->numel.at(nm);
    if (want != srcs[i].numel)
      VOG_FAIL(-3, "weight '%s': numel %lld, expected %lld", srcs[i].name, (long long)srcs[i].numel, (long long)want);
    given[nm] = srcs[i].dev;
  }
  std::vector<const WImage*> todo;
  const WImage* table = nullptr;
  for (const WImage& m : c->images) {
    int have = 0;
    for (auto& s : m.srcs) have += (int)given.count(s);
    if (have == 0) continue;
    if (have != (int)m.srcs.size())
      for (auto& s : m.srcs)
        if (!given.count(s))
          VOG_FAIL(-3, "image '%s' is built from %d weights and '%s' is not among the sources given", m.name.c_str(),
                   (int)m.srcs.size(), s.c_str());
    if (m.kind == VOG_IMG_GATE_TABLE) table = &m; else todo.push_back(&m);
  }
  const int R = c->d.rnn_size, E0 = c->d.emb_dim, et = c->d.enc_dtype;
  if (c->gx0_tab && !c->gx_wperm) {        // first refresh of this context: the gate table's operands live from here on
    VOG_HIP(hipMalloc((void**)&c->gx_wperm, (size_t)8 * R * E0 * 2));
    VOG_HIP(hipMalloc((void**)&c->gx_bperm, (size_t)8 * R * 4));
  }
  for (const WImage* m : todo) {
    WpackImage g = m->g;
    for (size_t s = 0; s < m->srcs.size() && s < 4; ++s) g.src[s] = given.at(m->srcs[s]);
    VOG_TRY(wpack_launch(g, st));
  }
  if (table) {
    // emb16 is an image of its own (already rewritten above, same stream); the other two operands in gate-table order,
    // then the GEMM vog_ctx_finalize runs
    WpackImage w = wimg(WL_PLAIN, WV_GATE, et, 0, 8 * R, E0, E0); w.R = R;
    w.dst = c->gx_wperm; w.bytes = (int64_t)8 * R * E0 * 2;
    w.src[0] = given.at(table->srcs[0]); w.src[1] = given.at(table->srcs[1]);
    VOG_TRY(wpack_launch(w, st));
    WpackImage b = wimg(WL_PLAIN, WV_GATE_BIAS, -1, 0, 1, 8 * R, 0); b.R = R;
    b.dst = c->gx_bperm; b.bytes = (int64_t)8 * R * 4;
    for (int s = 0; s < 4; ++s) b.src[s] = given.at(table->srcs[2 + s]);
    VOG_TRY(wpack_launch(b, st));
    const int64_t rows = (int64_t)c->d.vocab_size + 1, cols = (int64_t)8 * R;
    vog_gemm_args ga{}; ga.c16_dtype = -1;
    ga.a = c->emb16; ga.a_is_f32 = 0; ga.lda = E0; ga.K = E0;
    ga.w = c->gx_wperm; ga.ldw = E0; ga.bias = c->gx_bperm; ga.c32 = c->gx0_tab; ga.ldc = cols;
    ga.M = (int)rows; ga.N = (int)cols; ga.rep = 1; ga.dtype = (vog_dtype)et;
    VOG_TRY(vog_gemm_bias_act(&ga, st));
  }
  for (auto& kv : given) c->stale.insert(kv.first);
  return 0;
}

extern "C" int vog_ctx_finalize(vog_ctx* c) {
  VOG_CHECK_ARG(c);
  for (auto& n : c->names)
    if (!c->host.count(n)) VOG_FAIL(-3, "missing weight '%s'", n.c_str());
  // a device refresh went past the host copies: rebuilding from them would silently bring old values back
  for (auto& n : c->names)
    if (c->stale.count(n))
      VOG_FAIL(-3, "weight '%s' was refreshed on the device (vog_ctx_refresh_device): its host copy is stale, "
               "supply it again with vog_ctx_set_weight before vog_ctx_finalize", n.c_str());
  for (void* p : c->allocs) (void)hipFree(p);
  c->allocs.clear();
  c->images.clear();
  c->wih.clear(); c->wih_f.clear(); c->whh.clear(); c->bsum.clear(); c->wih_p.clear();
  c->obj = TxWeights(); c->mul = TxWeights();
  const vog_model_desc& d = c->d;
  const int R = d.rnn_size, et = d.enc_dtype;
  const std::string emb_n = "lstm_encoder.embed_tokens.weight";
  VOG_TRY(up32(c, emb_n, &c->emb, "emb"));
  VOG_TRY(up16(c, emb_n, d.enc_dtype, &c->emb16, "emb16"));
  for (int l = 0; l < d.rnn_layers; ++l) {
    const int in = l == 0 ? d.emb_dim : 2 * R;
    std::vector<unsigned short> whh((size_t)8 * R * R);
    std::vector<float> wcat((size_t)8 * R * in), bs((size_t)8 * R);       // both directions: W_ih rows, b_ih + b_hh
    int dir = 0;
    for (const char* sfx : {"", "_reverse"}) {
      std::string s = "_l" + std::to_string(l) + sfx;
      const auto& a = W(c, "lstm_encoder.lstm.weight_ih" + s);
      const auto& bi = W(c, "lstm_encoder.lstm.bias_ih" + s);
      const auto& bh = W(c, "lstm_encoder.lstm.bias_hh" + s);
      memcpy(&wcat[(size_t)dir * 4 * R * in], a.data(), a.size() * sizeof(float));
      for (int i = 0; i < 4 * R; ++i) bs[(size_t)dir * 4 * R + i] = bi[i] + bh[i];
      ++dir;
    }
    const std::string s0 = "_l" + std::to_string(l), s1 = s0 + "_reverse";
    VOG_TRY(vog_lstm_pack_whh(W(c, "lstm_encoder.lstm.weight_hh" + s0).data(),
                              W(c, "lstm_encoder.lstm.weight_hh" + s1).data(), whh.data(), R, (vog_dtype)et));
    unsigned short *pp = nullptr, *pf = nullptr, *pw, *ph; float* pb;
    const std::string im = "lstm." + std::to_string(l) + ".", lw = "lstm_encoder.lstm.";
    const std::vector<std::string> ih_src = {lw + "weight_ih" + s0, lw + "weight_ih" + s1};
    auto cat = [&](int layout, int K) { WpackImage g = wimg(layout, WV_CAT, et, 0, 8 * R, K, K); g.R = R; return g; };
    if (in % 256 == 0 && R % 32 == 0) {
      std::vector<unsigned short> wp((size_t)8 * R * in);
      VOG_TRY(vog_lstm_pack_w(W(c, "lstm_encoder.lstm.weight_ih" + s0).data(),
                              W(c, "lstm_encoder.lstm.weight_ih" + s1).data(), wp.data(), R, in, (vog_dtype)et));
      VOG_TRY(upload<unsigned short>(c, wp, &pp));
      rec(c, im + "wih_p", VOG_IMG_LSTM_PACK, pp, cat(WL_LSTM, in), ih_src);
    }
    c->wih_p.push_back(pp);
    if (in % 32 == 0) {
      std::vector<unsigned short> wf((size_t)8 * R * in);
      VOG_TRY(vog_pack_w_frag(wcat.data(), in, 8 * R, in, wf.data(), (vog_dtype)et));
      VOG_TRY(upload<unsigned short>(c, wf, &pf));
      rec(c, im + "wih_f", VOG_IMG_FRAG16, pf, cat(WL_FRAG16, in), ih_src);
    }
    c->wih_f.push_back(pf);
    VOG_TRY(upload<unsigned short>(c, to16(wcat, et), &pw));
    rec(c, im + "wih", VOG_IMG_WIH_CAT, pw, cat(WL_PLAIN, in), ih_src);
    VOG_TRY(upload<unsigned short>(c, whh, &ph));
    rec(c, im + "whh", VOG_IMG_LSTM_PACK, ph, cat(WL_LSTM, R), {lw + "weight_hh" + s0, lw + "weight_hh" + s1});
    VOG_TRY(upload<float>(c, bs, &pb));
    {
      WpackImage g = wimg(WL_PLAIN, WV_BIAS, -1, 0, 1, 8 * R, 0); g.R = R;
      rec(c, im + "bsum", VOG_IMG_BIAS_SUM, pb, g, {lw + "bias_ih" + s0, lw + "bias_hh" + s0, lw + "bias_ih" + s1, lw + "bias_hh" + s1});
    }
    c->wih.push_back(pw); c->whh.push_back(ph); c->bsum.push_back(pb);
  }
  // Gate table of layer 0 (round 6): G[v] = emb[v] . W_ih_l0^T + b_ih + b_hh for every token v and both directions - the input
  // projection of layer 0 depends on the token alone, so it is computed ONCE per checkpoint for the whole vocabulary (the same
  // 16-bit operands and fp32 accumulation the per-batch projection used) and a forward reads Bn x T rows of it (vog_lstm_layer_args.gx_table).
  // 164 MB at vocab 5000, R = 1024: sized for 288 GB of HBM. VOG_GX_TABLE_MAX_MB bounds it (default 2048; 0 = never).
  c->gx0_tab = nullptr;
  {
    const int64_t rows = (int64_t)d.vocab_size + 1, cols = (int64_t)8 * R;
    static const int64_t max_mb = getenv("VOG_GX_TABLE_MAX_MB") ? atoll(getenv("VOG_GX_TABLE_MAX_MB")) : 2048;
    if (c->emb16 && rows > 64 && (d.emb_dim % 64) == 0 && rows * cols * 4 <= max_mb * (1ll << 20) && vog_bilstm_layer_supported(1, R)) {
      float* tab = nullptr;
      VOG_HIP(hipMalloc(&tab, (size_t)(rows * cols * 4)));
      c->allocs.push_back(tab);
      // table column (dir, unit, gate): the four gates of a unit adjacent (one 16-byte read per lane of the layer kernel) -
      // W_ih rows and biases permuted accordingly for the one GEMM that builds it
      const int E0 = d.emb_dim;
      std::vector<unsigned short> wperm((size_t)8 * R * E0);
      std::vector<float> bperm((size_t)8 * R);
      {
        int dd = 0;
        for (const char* sfx : {"", "_reverse"}) {
          const auto& a = W(c, std::string("lstm_encoder.lstm.weight_ih_l0") + sfx);
          const auto& bi = W(c, std::string("lstm_encoder.lstm.bias_ih_l0") + sfx);
          const auto& bh = W(c, std::string("lstm_encoder.lstm.bias_hh_l0") + sfx);
          for (int r = 0; r < 4; ++r)
            for (int u = 0; u < R; ++u) {
              const size_t dst = (size_t)dd * 4 * R + (size_t)u * 4 + r, src = (size_t)r * R + u;
              bperm[dst] = bi[src] + bh[src];
              for (int k = 0; k < E0; ++k) wperm[dst * E0 + k] = h_to16(a[src * E0 + k], et);
            }
          ++dd;
        }
      }
      unsigned short* wp_d = nullptr; float* bp_d = nullptr;
      VOG_HIP(hipMalloc(&wp_d, wperm.size() * 2));
      VOG_HIP(hipMalloc(&bp_d, bperm.size() * 4));
      VOG_HIP(hipMemcpy(wp_d, wperm.data(), wperm.size() * 2, hipMemcpyHostToDevice));
      VOG_HIP(hipMemcpy(bp_d, bperm.data(), bperm.size() * 4, hipMemcpyHostToDevice));
      vog_gemm_args ga{}; ga.c16_dtype = -1;
      ga.a = c->emb16; ga.a_is_f32 = 0; ga.lda = E0; ga.K = E0;
      ga.w = wp_d; ga.ldw = E0; ga.bias = bp_d; ga.c32 = tab; ga.ldc = cols;
      ga.M = (int)rows; ga.N = (int)cols; ga.rep = 1; ga.dtype = (vog_dtype)et;
      const int grc = vog_gemm_bias_act(&ga, nullptr);
      VOG_HIP(hipStreamSynchronize(nullptr));
      (void)hipFree(wp_d); (void)hipFree(bp_d);
      if (grc != 0) return grc;
      c->gx0_tab = tab;
      {
        // (the GEMM's operands: emb16 and, in gate-table order, W_ih_l0 and the bias sums - WV_GATE / WV_GATE_BIAS)
        const std::string lw = "lstm_encoder.lstm.";
        WpackImage g = wimg(WL_PLAIN, WV_GATE, -1, 0, (int)rows, cols, cols); g.R = R;
        rec(c, "gx0_tab", VOG_IMG_GATE_TABLE, tab, g,
            {lw + "weight_ih_l0", lw + "weight_ih_l0_reverse", lw + "bias_ih_l0", lw + "bias_hh_l0", lw + "bias_ih_l0_reverse",
             lw + "bias_hh_l0_reverse", emb_n});
      }
    }
  }
  VOG_TRY(up16(c, "lstm_out_feat_proj.0.weight", et, &c->w_outproj, "w_outproj"));
  c->w_outproj_f = nullptr;
  if (d.lang_enc % 16 == 0) {
    std::vector<unsigned short> wf((size_t)d.lang_enc * 2 * R);
    VOG_TRY(vog_pack_w_frag(W(c, "lstm_out_feat_proj.0.weight").data(), 2 * R, d.lang_enc, 2 * R, wf.data(), (vog_dtype)et));
    VOG_TRY(upload<unsigned short>(c, wf, &c->w_outproj_f));
    rec(c, "w_outproj_f", VOG_IMG_FRAG16, c->w_outproj_f, wimg(WL_FRAG16, WV_DIRECT, et, 0, d.lang_enc, 2 * R, 2 * R),
        {"lstm_out_feat_proj.0.weight"});
  }
  VOG_TRY(up32(c, "lstm_out_feat_proj.0.bias", &c->b_outproj, "b_outproj"));
  VOG_TRY(up16(c, "prop_encoder.0.weight", et, &c->w_prop, "w_prop"));
  VOG_TRY(up32(c, "prop_encoder.0.bias", &c->b_prop, "b_prop"));
  VOG_TRY(up16(c, "seg_encoder.0.weight", et, &c->w_seg, "w_seg"));
  c->w_prop_f = c->w_seg_f = nullptr;
  if (vis_encode_supported(d.prop_dim, d.seg_dim, d.prop_enc, d.seg_enc)) {
    std::vector<unsigned short> wf((size_t)d.prop_enc * d.prop_dim), ws((size_t)d.seg_enc * d.seg_dim);
    VOG_TRY(vog_pack_w_frag(W(c, "prop_encoder.0.weight").data(), d.prop_dim, d.prop_enc, d.prop_dim, wf.data(), (vog_dtype)et));
    VOG_TRY(vog_pack_w_frag(W(c, "seg_encoder.0.weight").data(), d.seg_dim, d.seg_enc, d.seg_dim, ws.data(), (vog_dtype)et));
    VOG_TRY(upload<unsigned short>(c, wf, &c->w_prop_f));
    VOG_TRY(upload<unsigned short>(c, ws, &c->w_seg_f));
    auto enc_img = [&](int lo, int N, int K) { return wimg(WL_FRAG16, WV_DIRECT, et, lo, N, K, K); };
    rec(c, "w_prop_f", VOG_IMG_FRAG16, c->w_prop_f, enc_img(0, d.prop_enc, d.prop_dim), {"prop_encoder.0.weight"});
    rec(c, "w_seg_f", VOG_IMG_FRAG16, c->w_seg_f, enc_img(0, d.seg_enc, d.seg_dim), {"seg_encoder.0.weight"});
    c->w_prop_f_lo = c->w_seg_f_lo = nullptr;
    if (c->tx_split) {
      const auto& wp = W(c, "prop_encoder.0.weight");
      const auto& wsg = W(c, "seg_encoder.0.weight");
      VOG_TRY(vog_pack_w_frag(remainder16(wp.data(), wp.size(), et).data(), d.prop_dim, d.prop_enc, d.prop_dim, wf.data(), (vog_dtype)et));
      VOG_TRY(vog_pack_w_frag(remainder16(wsg.data(), wsg.size(), et).data(), d.seg_dim, d.seg_enc, d.seg_dim, ws.data(), (vog_dtype)et));
      VOG_TRY(upload<unsigned short>(c, wf, &c->w_prop_f_lo));
      VOG_TRY(upload<unsigned short>(c, ws, &c->w_seg_f_lo));
      rec(c, "w_prop_f_lo", VOG_IMG_FRAG16, c->w_prop_f_lo, enc_img(1, d.prop_enc, d.prop_dim), {"prop_encoder.0.weight"});
      rec(c, "w_seg_f_lo", VOG_IMG_FRAG16, c->w_seg_f_lo, enc_img(1, d.seg_enc, d.seg_dim), {"seg_encoder.0.weight"});
    }
  }
  VOG_TRY(up32(c, "seg_encoder.0.bias", &c->b_seg, "b_seg"));
  VOG_TRY(up16(c, "lin2.0.weight", et, &c->w_lin2, "w_lin2"));
  VOG_TRY(up32(c, "lin2.0.bias", &c->b_lin2, "b_lin2"));
  c->w_lin2_p = nullptr;
  {
    const int dm = d.prop_enc + d.seg_enc + d.lang_enc;
    if (has_mul(d) && tx_tail_supported(dm, dm / 2, 384)) {  // (a kwo every width takes: only d / dh are in question here)
      VOG_TRY(up_frag32(c, W(c, "lin2.0.weight").data(), dm, 256, dm, et, &c->w_lin2_p));
      rec(c, "w_lin2_p", VOG_IMG_FRAG32, c->w_lin2_p, wimg(WL_FRAG32, WV_DIRECT, et, 0, 256, dm, dm), {"lin2.0.weight"});
    }
  }
  VOG_TRY(up32(c, "lin2.2.weight", &c->w_lin2b, "w_lin2b"));
  VOG_TRY(up32(c, "lin2.2.bias", &c->b_lin2b, "b_lin2b"));
  VOG_TRY(up32(c, "srl_arg_words_out_enc.0.weight", &c->w_arg, "w_arg"));
  VOG_TRY(up32(c, "srl_arg_words_out_enc.0.bias", &c->b_arg, "b_arg"));
  VOG_TRY(up32(c, "seg_verb_classf.0.weight", &c->w_sv0, "w_sv0"));
  VOG_TRY(up32(c, "seg_verb_classf.0.bias", &c->b_sv0, "b_sv0"));
  VOG_TRY(up32(c, "seg_verb_classf.2.weight", &c->w_sv2, "w_sv2"));
  VOG_TRY(up32(c, "seg_verb_classf.2.bias", &c->b_sv2, "b_sv2"));
  const int d_obj = d.prop_enc + d.seg_enc, d_mul = d_obj + d.lang_enc;
  if (has_obj(d))
    VOG_TRY(finalize_tx(c, "obj_txf", "pe_obj_sub_enc.0", d_obj, d.obj_heads, d.obj_layers, d.obj_use_rel, &c->obj));
  if (has_mul(d))
    VOG_TRY(finalize_tx(c, "mult_txf", "pe_mul_sub_enc.0", d_mul, d.mul_heads, d.mul_layers, d.mul_use_rel, &c->mul));
  VOG_HIP(hipDeviceSynchronize());
  c->finalized = true;
  return 0;
}

extern "C" int vog_ctx_destroy(vog_ctx* c) {
  if (!c) return 0;
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->gx_wperm) (void)hipFree(c->gx_wperm);
  if (c->gx_bperm) (void)hipFree(c->gx_bperm);
  delete c;
  return 0;
}

extern "C" int64_t vog_workspace_bytes(const vog_ctx* c, int B, int ncmp, int T) {
  if (!c || !c->finalized || B <= 0 || ncmp <= 0 || T <= 0) return -1;
  return make_plan(c, make_geo(c->d, B, ncmp, T)).total;
}

// Can this model run with hi + lo operands (option tx_split) at `ncmp` videos per query? The kernels that carry the three-MFMA
// products: fused feature encoders (stream form; the segment replicas of many-proposal models by the copy step), the LDS-DMA QKV
// GEMM, attention of any length whose K + K remainder ring fits the LDS (plain: attn_sb / attn_frag_lean / attn_tile; structured
// mul_tx layer 0: one visual key block or the LDS-ring form), the fused encoder-layer tails.
extern "C" int vog_ctx_split_supported(const vog_ctx* c, int ncmp) {
  if (!c || ncmp <= 0) return 0;
  const vog_model_desc& d = c->d;
  if (!has_obj_weights(d)) return 0;                                   // ImgGrnd: no attention at all
  if (!vis_encode_supported(d.prop_dim, d.seg_dim, d.prop_enc, d.seg_enc)) return 0;
  if (d.nppf0 > 16 && ((d.seg_enc % 4) != 0 || (d.prop_enc % 4) != 0)) return 0;      // (the segment replicas: seg_rep)
  const Geo g = make_geo(d, 4, ncmp, 1);
  const int d_obj = d.prop_enc + d.seg_enc, d_mul = d_obj + d.lang_enc;
  auto tx_ok = [&](int dm, int H, int N) {
    const int chunk = (dm + H - 1) / H, dp = attn_head_pad(chunk);
    return dp > 0 && tx_tail_split_supported(dm, dm / 2, H * dp) && (dm % 64) == 0 && attn_split_supported(N, dp);
  };
  if (has_obj(d) && !tx_ok(d_obj, d.obj_heads, g.N_obj)) return 0;
  if (has_mul(d)) {
    if ((d_obj % 64) != 0 || (d.lang_enc % 32) != 0) return 0;                      // structured layer 0
    if (!tx_ok(d_mul, d.mul_heads, d.mul_layers > 1 ? g.N_mul : 1)) return 0;
    if (!attn_struct_split_supported(g.nppf, d.nsrl, attn_head_pad((d_mul + d.mul_heads - 1) / d.mul_heads))) return 0;
  }
  return 1;
}

static int workspace_zero(const vog_ctx* c, int64_t need, void* ws, size_t ws_bytes, void* stream, const char* what) {
  VOG_CHECK_ARG(c && ws);
  if (need < 0 || (int64_t)ws_bytes < need) VOG_FAIL(-2, "%s too small", what);
  VOG_HIP(hipMemsetAsync(ws, 0, (size_t)need, (hipStream_t)stream));
  return 0;
}

extern "C" int vog_workspace_init(const vog_ctx* c, int B, int ncmp, int T, void* ws, size_t ws_bytes,
                                  void* stream) {
  return workspace_zero(c, vog_workspace_bytes(c, B, ncmp, T), ws, ws_bytes, stream, "workspace");
}

extern "C" int vog_workspace_stage(const vog_ctx* c, int B, int ncmp, int T, const char* stage,
                                   int64_t* offset, int64_t* bytes) {
  VOG_CHECK_ARG(c && c->finalized && stage && offset && bytes);
  Plan p = make_plan(c, make_geo(c->d, B, ncmp, T));
  auto it = p.buf.find(stage);
  if (it == p.buf.end()) VOG_FAIL(-4, "no stage '%s'", stage);
  *offset = it->second.first;
  *bytes = it->second.second;
  return 0;
}

// ---- group language encoder -------------------------------------------------------------------
extern "C" int64_t vog_lang_workspace_bytes(const vog_ctx* c, int B, int ncmp, int T) {
  if (!c || !c->finalized || B <= 0 || ncmp <= 0 || T <= 0) return -1;
  return make_plan(c, make_geo(c->d, B, ncmp, T), true).total;
}

extern "C" int vog_lang_workspace_init(const vog_ctx* c, int B, int ncmp, int T, void* ws, size_t ws_bytes,
                                       void* stream) {
  return workspace_zero(c, vog_lang_workspace_bytes(c, B, ncmp, T), ws, ws_bytes, stream, "language workspace");
}

extern "C" int vog_lang_outputs(const vog_ctx* c, int B, int ncmp, int T, void* ws, float** lang,
                                float** final_hidden) {
  VOG_CHECK_ARG(c && c->finalized && ws && B > 0 && ncmp > 0 && T > 0);
  const Geo g = make_geo(c->d, B, ncmp, T);
  Plan p = make_plan(c, g, true);
  WS w{(char*)ws, &p};
  if (lang) *lang = w.at<float>("lang");
  if (final_hidden) *final_hidden = w.at<float>("full") + (int64_t)g.Bn * g.T * g.L;
  return 0;
}

extern "C" int vog_lang_forward(vog_ctx* c, const vog_batch* lb, void* ws, size_t ws_bytes, void* stream) {
  VOG_CHECK_ARG(c && lb && ws);
  Plan plan;
  std::vector<Step> steps;
  VOG_TRY(build_steps(c, lb, ws, ws_bytes, plan, steps, true));
  return run_steps(steps, (hipStream_t)stream);
}

// LSTMEncoder.forward (utils/mdl_srl_utils.py:114-169) on its own: token re-index + embedding + the packed 2-layer BiLSTM,
// both layers, both directions - the language chain of the forward up to (not including) lstm_out_feat_proj.
extern "C" int vog_bilstm_fwd(vog_ctx* c, const vog_batch* lb, void* ws, size_t ws_bytes, float* x_out, float* final_hidden,
                              void* stream) {
  VOG_CHECK_ARG(c && lb && ws && x_out && final_hidden);
  Plan plan;
  std::vector<Step> steps;
  VOG_TRY(build_steps(c, lb, ws, ws_bytes, plan, steps, true));
  for (auto& s : steps) {
    const bool lstm_part = s.name == "prep" || s.name == "lang_prep" || s.name.rfind("lstm_ih", 0) == 0 ||
                           s.name == "lstm_layer" || s.name == "lstm_step";
    if (lstm_part) VOG_TRY(s.fn((hipStream_t)stream));
  }
  const Geo g = make_geo(c->d, lb->B, lb->ncmp, lb->T);
  WS w{(char*)ws, &plan};
  const int top = c->d.rnn_layers - 1;
  const bool ofrag = make_lstm_form(c, g).out_frag[top];
  return vog_lstm_out_to_f32(w.at<void>("lstm_out16_" + std::to_string(top)), ofrag ? 1 : 0, g.Bn * g.T, g.Bn, 2 * g.R,
                             (vog_dtype)c->d.enc_dtype, x_out, final_hidden, stream);
}

namespace vog {
// steps of a whole group: [language chain] + members' forwards; member_of[i] = -1 for language steps
static int build_group(vog_ctx* c, const vog_batch* lb, void* lws, size_t lbytes, const vog_batch* const* members,
                       void* const* wss, const size_t* wbytes, int n, std::vector<Step>& steps,
                       std::vector<int>& member_of) {
  VOG_CHECK_ARG(c && lb && lws && members && wss && wbytes && n >= 1 && n <= 16);
  Plan lp;
  VOG_TRY(build_steps(c, lb, lws, lbytes, lp, steps, true));
  member_of.assign(steps.size(), -1);
  int b_sum = 0;
  for (int m = 0; m < n; ++m) {
    VOG_CHECK_ARG(members[m] && wss[m] && members[m]->shared_lang && members[m]->ncmp == lb->ncmp);
    b_sum += members[m]->B;
    Plan mp;
    std::vector<Step> ms;
    VOG_TRY(build_steps(c, members[m], wss[m], wbytes[m], mp, ms));
    steps.insert(steps.end(), ms.begin(), ms.end());
    member_of.resize(steps.size(), m);
  }
  if (b_sum != lb->B) VOG_FAIL(-1, "group: members hold %d queries, the language batch %d", b_sum, lb->B);
  return 0;
}
}  // namespace vog

extern "C" int vog_group_forward(vog_ctx* c, const vog_batch* lb, void* lws, size_t lbytes,
                                 const vog_batch* const* members, void* const* wss, const size_t* wbytes,
                                 int n, void* stream) {
  std::vector<Step> steps;
  std::vector<int> mo;
  VOG_TRY(vog::build_group(c, lb, lws, lbytes, members, wss, wbytes, n, steps, mo));
  return run_steps(steps, (hipStream_t)stream);
}

extern "C" int vog_forward(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, void* stream) {
  VOG_CHECK_ARG(c && b && ws);
  Plan plan;
  std::vector<Step> steps;
  VOG_TRY(build_steps(c, b, ws, ws_bytes, plan, steps));
  return run_steps(steps, (hipStream_t)stream);               // eager: one stream, program order (re-entrant)
}

extern "C" int vog_ctx_encode_videos(vog_ctx* c, int B_like, int ncmp_like, const float* prop, const float* seg,
                                     float* enc_prop_out, float* enc_seg_out, void* ws, size_t ws_bytes, void* stream) {
  VOG_CHECK_ARG(c);
  if (B_like <= 0 || ncmp_like <= 0) VOG_FAIL(-1, "vog_ctx_encode_videos: geometry %d x %d", B_like, ncmp_like);
  VOG_CHECK_ARG(prop && seg && enc_prop_out && enc_seg_out && ws);
  VOG_CHECK_ARG(c->finalized);
  const vog_model_desc& d = c->d;
  const Geo g = make_geo(d, B_like, ncmp_like, 1);
  Plan plan = make_plan(c, g);
  if ((int64_t)ws_bytes < plan.total) VOG_FAIL(-2, "workspace too small: %zu < %lld", ws_bytes, (long long)plan.total);
  vog_batch b{};
  b.B = B_like; b.ncmp = ncmp_like; b.T = 1;
  b.pad_region_feature = prop; b.seg_feature_for_frms = seg;
  // the builder of a forward of this geometry decides the form of the encoders (every flag it reads is the context's or the
  // geometry's); only its encoder stage is emitted, with the feature cast the prologue would have done in front of the GEMM form
  std::vector<Step> steps;
  Builder B(c, &b, g, WS{(char*)ws, &plan}, steps, false, true);
  if (!B.enc_fused) {
    vog_visprep_args vp{};
    vp.src0 = prop; vp.dst0 = B.ws.at<void>("prop16"); vp.n0 = g.rows_obj * d.prop_dim;
    vp.src1 = seg; vp.dst1 = B.ws.at<void>("seg16"); vp.n1 = (int64_t)g.n_vid * g.Fv * d.seg_dim;
    vp.dtype = (vog_dtype)d.enc_dtype;
    B.vis("vis_prep", [vp](hipStream_t st) { return vog_vis_prep(&vp, st); });
  }
  VOG_TRY(B.raw_encoder_steps());
  VOG_TRY(run_steps(steps, (hipStream_t)stream));
  return vis_split_run(B.ws.at<float>("prop_seg"), g.d_obj, enc_prop_out, enc_seg_out, (int)g.rows_obj, d.nppf0, d.prop_enc,
                       d.seg_enc, (hipStream_t)stream);
}

extern "C" int vog_ctx_obj_band_rows(const vog_ctx* c) {
  if (!c || !c->finalized || !has_obj(c->d)) return -1;
  const TxWeights& tw = c->obj;
  bool fused = c->fused_tail && tx_tail_supported(tw.d, tw.dh, tw.H * tw.dp);
  for (auto& l : tw.layers) fused = fused && l.wo_p;
  if (!fused) return 0;
  return (c->tx_split ? 32 : 64) * 8;       // (TxTailBody: xpos = (row block >> 3) & 7 picks the k-step rotation)
}

extern "C" int vog_ctx_set_stats(vog_ctx* c, uint32_t* stats) {
  VOG_CHECK_ARG(c);
  c->stats = stats;
  return 0;
}

extern "C" int vog_ctx_obj_videos(vog_ctx* c, int B_like, int ncmp_like, const float* prop, const float* seg,
                                  const float* pad_proposals, float* obj_out, float* enc_seg_out, void* ws, size_t ws_bytes,
                                  void* stream) {
  VOG_CHECK_ARG(c);
  if (B_like <= 0 || ncmp_like <= 0) VOG_FAIL(-1, "vog_ctx_obj_videos: geometry %d x %d", B_like, ncmp_like);
  VOG_CHECK_ARG(prop && seg && pad_proposals && obj_out && enc_seg_out && ws);
  const vog_model_desc& d = c->d;
  if (d.conc_type != VOG_CONC_SEP || !has_obj(d))
    VOG_FAIL(-1, "vog_ctx_obj_videos needs a sep / svsq model with an object transformer (elsewhere obj_tx attends across the "
                 "videos of a query, or does not exist: vog_ctx_encode_videos already covers this model)");
  VOG_CHECK_ARG(c->finalized);
  const Geo g = make_geo(d, B_like, ncmp_like, 1);
  Plan plan = make_plan(c, g);
  if ((int64_t)ws_bytes < plan.total) VOG_FAIL(-2, "workspace too small: %zu < %lld", ws_bytes, (long long)plan.total);
  vog_batch b{};
  b.B = B_like; b.ncmp = ncmp_like; b.T = 1;
  b.pad_region_feature = prop; b.seg_feature_for_frms = seg; b.pad_proposals = pad_proposals;
  // the builder of a forward of this geometry decides the form of every step: the visual prologue on its own (feature cast
  // for the GEMM encoders, box-bias precursors), the encoder stage, the obj_tx stack
  std::vector<Step> steps;
  Builder B(c, &b, g, WS{(char*)ws, &plan}, steps, false, true);
  hipStream_t st = (hipStream_t)stream;
  // (the attention's per-layer guard words: a forward's prologue zero-fills them, vog_attn_args.guard_precleared)
  VOG_HIP(hipMemsetAsync(B.ws.at<void>("obj_guard"), 0, 256, st));
  const vog_visprep_args vp = B.visprep_args();
  B.vis("vis_prep", [vp](hipStream_t s) { return vog_vis_prep(&vp, s); });
  VOG_TRY(B.raw_encoder_steps());
  TxStackIO obj = B.obj_stack_io();
  VOG_TRY(B.tx_stack_steps(c->obj, "obj", obj));
  VOG_TRY(run_steps(steps, st));
  VOG_HIP(hipMemcpyAsync(obj_out, obj.out32, (size_t)g.rows_obj * g.d_obj * sizeof(float), hipMemcpyDeviceToDevice, st));
  VOG_TRY(vis_split_run(B.ws.at<float>("prop_seg"), g.d_obj, nullptr, enc_seg_out, (int)g.rows_obj, d.nppf0, d.prop_enc, d.seg_enc, st));
  if (c->stats)
    VOG_TRY(logit_fold_run(B.ws.at<unsigned int>("logit_max"), c->stats, B.ws.at<unsigned int>("logit_pub"), 1, st));
  return 0;
}

struct vog_graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

// Capture what `issue(stream)` launches on `stream` as one graph and instantiate it.
// One linear chain. (A DAG form - the language chain captured as a parallel branch - was measured and
// removed: graph branches of 4 forwards in flight oversubscribe the 4 hardware queues, 33 k instead of
// 48 k queries/s, and replaying two such graphs on 2 streams crashed inside hipGraphLaunch on ROCm 7.2.
// Steps that can run side by side share a launch instead: csrc/pair.hip.)
template <typename Issue>
static int capture_graph(hipStream_t st, Issue issue, vog_graph** out) {
  VOG_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = issue(st);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(st, &g);
  if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) VOG_FAIL(-(int)e - 1000, "hipStreamEndCapture: %s", hipGetErrorString(e));
  vog_graph* vg = new vog_graph();
  vg->graph = g;
  e = hipGraphInstantiate(&vg->exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); delete vg; VOG_FAIL(-(int)e - 1000, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
  *out = vg;
  return 0;
}

// the rest of a validation step on the forward's chain: loss, then metrics + the row of the logs
static int run_val_epilogue(const vog_val_epilogue* epi, hipStream_t st) {
  if (epi->loss) VOG_TRY(vog_loss_fwd(epi->loss, st));
  if (epi->metrics) {                                      // the log rides in the metrics launch
    vog_gmetric_args m = *epi->metrics;
    m.log = epi->log;
    return vog_ground_metrics(&m, st);
  }
  return vog_val_log(epi->log, st);
}

// The fed graph: the batch's way onto the device first (kernel nodes reading pinned host memory at fixed addresses, or a
// device staging buffer behind one transfer), then the forward, then what a validation step appends, all on one chain. The
// query-bank gather comes in front of the assembly: that reads its index and its per-query arrays from buffers the gather has
// just written (vid_index may itself be a column of the query bank).
static int capture_fed(const vog_fed_desc& d, void* stream, vog_graph** out) {
  VOG_CHECK_ARG(d.ctx && d.batch && d.ws && out && stream);
  VOG_CHECK_ARG(d.nseg >= 0 && d.nseg <= VOG_MAX_COPY_SEGS && (d.nseg == 0 || d.segs));
  VOG_CHECK_ARG(!(d.asm_args && d.bank_args) && (!d.epi || d.epi->log));
  Plan plan;
  std::vector<Step> steps;
  VOG_TRY(build_steps(d.ctx, d.batch, d.ws, d.ws_bytes, plan, steps));
  return capture_graph((hipStream_t)stream, [&](hipStream_t st) -> int {
    if (d.dma && d.dma->bytes) {
      hipError_t de = hipMemcpyAsync(d.dma->dst, d.dma->src, d.dma->bytes, hipMemcpyHostToDevice, st);
      if (de != hipSuccess) VOG_FAIL(-(int)de - 1000, "hipMemcpyAsync (fed graph): %s", hipGetErrorString(de));
    }
    if (d.gather) VOG_TRY(vog_gather_rows(d.gather, st));
    if (d.bank_args) VOG_TRY(vog_assemble_from_bank(d.bank_args, st));
    if (d.asm_args) VOG_TRY(vog_assemble_batch(d.asm_args, st));
    if (d.nseg > 0) VOG_TRY(vog_copy_segments(d.segs, d.nseg, st));
    VOG_TRY(run_steps(steps, st));
    return d.epi ? run_val_epilogue(d.epi, st) : 0;
  }, out);
}

extern "C" int vog_graph_capture_desc(const vog_fed_desc* d, void* stream, vog_graph** out) {
  VOG_CHECK_ARG(d);
  return capture_fed(*d, stream, out);
}

// shorthands for the descriptor
extern "C" int vog_graph_capture_val(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, const vog_copy_seg* dma,
                                     const vog_assemble_args* asm_args, const vog_bank_assemble_args* bank_args,
                                     const vog_copy_seg* segs, int nseg, const vog_val_epilogue* epi, void* stream,
                                     vog_graph** out) {
  VOG_CHECK_ARG(epi && epi->log && !(asm_args && bank_args));
  return capture_fed(vog_fed_desc{c, b, ws, ws_bytes, dma, nullptr, asm_args, bank_args, segs, nseg, epi}, stream, out);
}

extern "C" int vog_graph_capture_fed(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, const vog_copy_seg* dma,
                                     const vog_assemble_args* asm_args, const vog_copy_seg* segs, int nseg, void* stream,
                                     vog_graph** out) {
  return capture_fed(vog_fed_desc{c, b, ws, ws_bytes, dma, nullptr, asm_args, nullptr, segs, nseg, nullptr}, stream, out);
}

extern "C" int vog_graph_capture_fed_bank(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, const vog_copy_seg* dma,
                                          const vog_bank_assemble_args* bank_args, const vog_copy_seg* segs, int nseg,
                                          void* stream, vog_graph** out) {
  VOG_CHECK_ARG(bank_args);
  return capture_fed(vog_fed_desc{c, b, ws, ws_bytes, dma, nullptr, nullptr, bank_args, segs, nseg, nullptr}, stream, out);
}

extern "C" int vog_graph_capture(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes,
                                 void* stream, vog_graph** out) {
  return capture_fed(vog_fed_desc{c, b, ws, ws_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr}, stream, out);
}

extern "C" int vog_group_graph_capture(vog_ctx* c, const vog_batch* lb, void* lws, size_t lbytes,
                                       const vog_batch* const* members, void* const* wss,
                                       const size_t* wbytes, int n, void* stream, vog_graph** out) {
  VOG_CHECK_ARG(out && stream);
  std::vector<Step> steps;
  std::vector<int> mo;
  VOG_TRY(vog::build_group(c, lb, lws, lbytes, members, wss, wbytes, n, steps, mo));
  return capture_graph((hipStream_t)stream, [&](hipStream_t st) { return run_steps(steps, st); }, out);
}

extern "C" int vog_ctx_set_int(vog_ctx* c, const char* name, int value) {
  VOG_CHECK_ARG(c && name);
  if (strcmp(name, "tx_split") == 0) {        // takes effect at the next vog_ctx_finalize (the remainder weights are made there)
    if ((value != 0) != (c->tx_split != 0)) c->finalized = false;
    c->tx_split = value ? 1 : 0;
    return 0;
  }
  if (strcmp(name, "lstm_persistent") == 0) { c->lstm_persistent = value ? 1 : 0; return 0; }
  if (strcmp(name, "lstm_wide") == 0) { c->lstm_wide = value ? 1 : 0; return 0; }
  if (strcmp(name, "lstm_inject_stall") == 0) { c->lstm_inject_stall = value == 2 ? 2 : (value ? 1 : 0); return 0; }   // 2: direction 1 only
  if (strcmp(name, "fused_tail") == 0) { c->fused_tail = value ? 1 : 0; return 0; }
  if (strcmp(name, "fused_enc") == 0) { c->fused_enc = value ? 1 : 0; return 0; }
  if (strcmp(name, "pair_launches") == 0) { c->pair_launches = value ? 1 : 0; return 0; }
  if (strcmp(name, "pair_mask") == 0) { c->pair_mask = value & 15; return 0; }
  if (strcmp(name, "fused_ih") == 0) { c->fused_ih = value; return 0; }
  if (strcmp(name, "enc_lean") == 0) { c->enc_lean = value; return 0; }
  VOG_FAIL(-4, "unknown option '%s'", name);
}

extern "C" int vog_graph_launch(vog_graph* g, void* stream) {
  VOG_CHECK_ARG(g && g->exec);
  VOG_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
  return 0;
}

extern "C" int vog_graph_destroy(vog_graph* g) {
  if (!g) return 0;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
  return 0;
}

extern "C" int vog_describe_steps(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, int lang_only, char* out,
                                  size_t out_bytes) {
  VOG_CHECK_ARG(c && b && ws && out);
  Plan plan;
  std::vector<Step> steps;
  VOG_TRY(build_steps(c, b, ws, ws_bytes, plan, steps, lang_only != 0));
  std::string s;
  for (auto& x : steps) s += x.name + "\n";
  if (s.size() + 1 > out_bytes) VOG_FAIL(-2, "vog_describe_steps: %zu bytes needed, %zu given", s.size() + 1, out_bytes);
  memcpy(out, s.c_str(), s.size() + 1);
  return 0;
}

extern "C" int vog_time_kernel(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes,
                               const char* kernel, int iters, void* stream, float* usec) {
  VOG_CHECK_ARG(c && b && ws && kernel && iters > 0 && usec);
  Plan plan;
  std::vector<Step> steps;
  VOG_TRY(build_steps(c, b, ws, ws_bytes, plan, steps));
  // "name#k": the k-th step of that name (the two BiLSTM layers share one)
  std::string want(kernel);
  int occ = 0;
  { const size_t h = want.find('#'); if (h != std::string::npos) { occ = atoi(want.c_str() + h + 1); want.resize(h); } }
  const Step* s = nullptr;
  auto pick = [&]() { int k = occ; for (auto& x : steps) if (x.name == want && k-- == 0) { s = &x; break; } };
  pick();
  if (!s) {     // a step that runs paired in the forward can still be timed on its own
    steps.clear();
    VOG_TRY(build_steps(c, b, ws, ws_bytes, plan, steps, false, false));
    pick();
  }
  if (!s) VOG_FAIL(-4, "no kernel step '%s'", kernel);
  hipStream_t st = (hipStream_t)stream;
  // the persistent layer kernel consumes per-forward state (hand-off tags zeroed by lang_prep):
  // time (lang_prep + layer) pairs and subtract lang_prep timed alone the same way
  const Step* reset = nullptr;
  if (s->name.rfind("lstm_layer", 0) == 0)
    for (auto& x : steps) if (x.name == "lang_prep" || x.name == "prep") { reset = &x; break; }
  struct Events {     // destroyed on every path out of here
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ev;
  VOG_HIP(hipEventCreate(&ev.e0));
  VOG_HIP(hipEventCreate(&ev.e1));
  auto timed = [&](const Step* a, const Step* b2, float* out_ms) -> int {
    for (int i = 0; i < 3; ++i) { if (a) VOG_TRY(a->fn(st)); if (b2) VOG_TRY(b2->fn(st)); }
    VOG_HIP(hipEventRecord(ev.e0, st));
    for (int i = 0; i < iters; ++i) { if (a) VOG_TRY(a->fn(st)); if (b2) VOG_TRY(b2->fn(st)); }
    VOG_HIP(hipEventRecord(ev.e1, st));
    VOG_HIP(hipEventSynchronize(ev.e1));
    VOG_HIP(hipEventElapsedTime(out_ms, ev.e0, ev.e1));
    return 0;
  };
  float ms = 0.f, ms_reset = 0.f;
  VOG_TRY(timed(reset, s, &ms));
  if (reset) VOG_TRY(timed(reset, nullptr, &ms_reset));
  *usec = (ms - ms_reset) * 1000.0f / (float)iters;
  return 0;
}
