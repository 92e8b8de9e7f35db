/*
 * vog_hip.h — C ABI of libvog_hip.so: the MI355X (gfx950) engine underneath the
 * VOGNet forward path.
 *
 * The reference (TheShadow29/vognet-pytorch) has no FFI: its plugin boundary is
 * the Python surface `get_mdl_loss_eval(cfg)` (code/mdl_selector.py:26-69),
 * `cls(cfg, comm)` (code/mdl_base.py:11-22) and `forward(dict) -> dict`
 * (code/mdl_conc_single.py:68-127, code/mdl_conc_sep.py:131-217). The build
 * keeps that surface in `vognet-pytorch_amd/` and binds THIS library under it
 * with ctypes. Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - every entry returns int: 0 = ok, <0 = error (message: vog_last_error()).
 *   - tensors are raw DEVICE pointers + explicit sizes; the caller owns every
 *     buffer (inputs, outputs, workspace). No allocation, no hidden sync and no
 *     global mutable state on the launch path => re-entrant across streams.
 *   - `stream` is a hipStream_t passed as void* (torch: current_stream().cuda_stream).
 *   - 16-bit tensors ("t16") are raw bf16 or IEEE f16 bit patterns, selected by
 *     a vog_dtype argument; accumulation is always fp32.
 *   - weights are HOST fp32 pointers handed over once (vog_ctx_set_weight) under
 *     the reference's state_dict key names (utils/trn_utils.py:534-593 loads
 *     exactly these keys), uploaded / converted / padded by vog_ctx_finalize.
 */
#ifndef VOG_HIP_H
#define VOG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOG_ABI_VERSION 1

typedef enum { VOG_BF16 = 0, VOG_F16 = 1 } vog_dtype;
typedef enum { VOG_MDL_IGRND = 0, VOG_MDL_VGRND = 1, VOG_MDL_VOG = 2 } vog_mdl_kind;
/* svsq is SEP with ncmp = 1 */
typedef enum { VOG_CONC_SEP = 0, VOG_CONC_TEMP = 1, VOG_CONC_SPAT = 2 } vog_conc_type;

int vog_version(void);
const char* vog_last_error(void);

/* ------------------------------------------------------------------------- *
 * Operator level (one per hot-path kernel; used by the parity tests and by
 * vog_forward internally)
 * ------------------------------------------------------------------------- */

/* C = act(A * W^T + bias) [+ residual]   — replaces nn.Linear everywhere on the
 * path (transformer_code.py:58-61,77-81,169-172; mdl_vog.py:182-188,202-207,
 * 224-230). A: [M,K] fp32 (a_is_f32=1) or t16, row pitch lda; optional row
 * gather a_rows[M] (int32) — the embedding lookup of mdl_srl_utils.py:128.
 * W: [N,K] t16 row pitch ldw (K % 8 == 0). Outputs (either may be NULL):
 * c32 fp32 / c16 t16 (type c16_dtype), row pitch ldc; output row = m*rep + j for j < rep
 * (rep > 1 broadcasts a frame's segment feature onto its proposals,
 * mdl_conc_single.py:51-66). */
struct vog_vislang_args;
typedef struct vog_gemm_args {
  const void* a; int a_is_f32; int64_t lda; const int32_t* a_rows;
  const void* w; int64_t ldw;
  const float* bias;           /* [N] or NULL */
  const float* residual;       /* [M, ldr] fp32 or NULL (rep must be 1) */
  int64_t ldr;
  float* c32; void* c16; int64_t ldc; int64_t ldc16;
  int M, N, K; int relu; int rep; vog_dtype dtype;
  int c16_dtype;               /* vog_dtype of c16, or -1 = same as dtype */
  /* optional output-row scatter: column n belongs to segment n / out_rows_ncol and
   * row m of that segment is written to row out_rows[seg*M + m] (< 0: dropped).
   * Used to emit the LSTM input projections directly in (direction, step) order. */
  const int32_t* out_rows; int out_rows_ncol;
  /* optional implicit residual: the residual row of output row m is the vis||lang
   * token m of this layout (never materialised); `residual` must then be NULL. */
  const struct vog_vislang_args* res_vislang;
  /* split-K (> 1): the K range is cut into `splitk` slices, slice s writes its raw
   * partial product to c32 + s*M*ldc (fp32 slabs, plain stores); bias / relu /
   * residual / c16 / rep must be unset — apply them with vog_splitk_finish. For
   * GEMMs with fewer output tiles than CUs and a long K (the two feature encoders). */
  int splitk;
  /* w_frag = 1: `w` is in MFMA-fragment order (vog_pack_w_frag: [N/16][K/32][64 lanes][8],
   * one contiguous KiB per fragment) — only for the M <= 64 weight-streaming kernel
   * (K % 32 == 0, N % 16 == 0), where the row-major layout makes every wave load touch
   * 16 half-used cache lines. */
  int w_frag;
  /* a_frag = 1 (M <= 64 kernel only, 16-bit A): `a` is in fragment order
   * [m/16][K/32][lane = ((k%32)/8)*16 + m%16][k%8] — written that way by vog_bilstm_step
   * (out_frag) so that the LSTM -> projection hand-off needs no strided fragment loads. */
  int a_frag;
  /* round 6, optional (M <= 64 kernel, a_is_f32, w_frag): w_lo = the fragment-ordered 16-bit remainder t16(w - t16(w)) of the fp32
   * weights; the fp32 rows of `a` are split the same way in the kernel and the product is a.w + a_lo.w + a.w_lo (three MFMAs). */
  const void* w_lo;
} vog_gemm_args;
/* host: fp32 [N, ld] (first K columns) -> 16-bit fragment order, N*K halfwords. */
int vog_pack_w_frag(const float* w, int64_t ld, int N, int K, void* dst_host, vog_dtype dtype);
int vog_gemm_bias_act(const vog_gemm_args* g, void* stream);

/* out[m*rep + j, n] = act(sum_s slab[s][m][n] + bias[n]) for up to two problems in
 * one launch (prop_encoder + seg_encoder), fp32 and/or 16-bit outputs. */
typedef struct vog_splitk_prob {
  const float* slabs; int splits; int M, N; const float* bias; int relu; int rep;
  float* c32; void* c16; int64_t ldc, ldc16; int c16_dtype;
} vog_splitk_prob;
int vog_splitk_finish(const vog_splitk_prob* p0, const vog_splitk_prob* p1, void* stream);

/* Fused QKV projection for one (Rel)MultiHead (transformer_code.py:64-67,
 * 180-183): x[S*N, K] * Wqkv_pad^T where Wqkv_pad is [3*H*dp, K] (heads padded
 * to dp columns with zero rows, dp % 32 == 0). Writes q, k, v per (sequence, head)
 * in MFMA-FRAGMENT ORDER, npad*dp halfwords each, npad = N rounded up to 32:
 *   q/k : [token/32][dd/16][lane = ((dd/8)&1)*32 + token%32][dd%8]
 *   v   : [token/32][dd/32][(token%32)/16][lane = hi*32 + dd%32][j],
 *         token%16 = 8*(j>>2) + 4*hi + (j&3)
 * (csrc/common.h frag_qk / frag_v). Pad tokens are never written: zero the
 * buffers once (vog_workspace_init does). */
typedef struct vog_qkv_args {
  const void* x16; int64_t ldx; const void* wqkv; int64_t ldw;
  void* q; void* k; void* vt;
  int S, N, H, dp, npad, K; vog_dtype dtype;
  /* structured layer 0 of mul_tx (pl != NULL): x16 holds the n_vid*nfrm*nppf VISUAL rows
   * only ([rows, K = d_vis]), wqkv its first K columns (row pitch ldw); pl = lang Wqkv[:, d_vis:]^T
   * ([n_lang*nsrl, 3*H*dp] fp32). The epilogue emits, for every visual row and every one of
   * the nsrl arguments, token (arg*nppf + p) = projection + pl[lang row of that arg]:
   * S = n_vid*nfrm sequences of N = nsrl*nppf tokens, no [tokens, d] matrix and no fp32
   * intermediate in HBM (see vog_qkv_combine for the unfused form). */
  const float* pl; int nsrl, nppf, nfrm, lang_per_vid, nc_v;
  /* kv_visual_only = 1 (with pl): q is fanned out as above, but k and vt are written for the nppf
   * VISUAL tokens of every sequence only ([S,H,npad_kv*dp], no language part): the operands of
   * vog_rel_attention_struct_fwd. */
  int kv_visual_only, npad_kv;
  /* wqkv_p32 != NULL: row-block form for MANY rows (csrc/qkvrb_dev.h; p100): the same [3*H*dp, K] weights in vog_pack_w_frag32
   * order; one workgroup per 64 rows stages its rows in LDS once and walks all output columns, streaming each weight fragment
   * once. Needs vog_qkv_rowblock_supported(3*H*dp, K); wqkv / ldw are not read. */
  const void* wqkv_p32;
  /* round 6, hi + lo operands (optional; all four or none; plain form, pl == NULL): x16_lo = t16(x - t16(x)) of the fp32
   * activations ([rows, ldx] like x16), wqkv_lo the same of the fp32 weights ([3*H*dp, ldw] like wqkv); the projection is
   * x.w + x_lo.w + x.w_lo (three MFMAs) and Q / K are written as q + q_lo, k + k_lo (V^T as one 16-bit image). */
  const void* x16_lo; const void* wqkv_lo; void* q_lo; void* k_lo;
} vog_qkv_args;
int vog_qkv_proj(const vog_qkv_args* a, void* stream);
int vog_qkv_rowblock_supported(int n_out, int K);

/* Layer-0 QKV of mul_tx through the token structure: every token is
 * [vis[v, f*nppf+p] || lang[l, a]], so x Wqkv^T = PV[vis row] + PL[lang row] with
 * PV = vis Wqkv[:, :dv]^T ([n_vid*NP, 3*H*dp] fp32) and PL = lang Wqkv[:, dv:]^T
 * ([n_lang*nsrl, 3*H*dp] fp32): 5x fewer projection FLOPs than the dense
 * [tokens, d] GEMM of transformer_code.py:180 and no token matrix in HBM. This
 * entry adds the two parts (one rounding to 16 bit) and emits q, k, v in the
 * fragment order of vog_qkv_proj. */
typedef struct vog_qkvcomb_args {
  const float* pv; const float* pl; void* q; void* k; void* vt;
  int n_vid, nfrm, nppf, nsrl, H, dp, npad; int lang_per_vid, nc_v; vog_dtype dtype;
} vog_qkvcomb_args;
int vog_qkv_combine(const vog_qkvcomb_args* a, void* stream);

/* softmax((q k^T + bias)/scale) v per (sequence, head), flash-style, with the
 * relative-position bias computed on the fly: bias[i,j] = relu(u[i]-u[j]+pe_b[h])
 * where u[token,h] = W_pe[h,:].box_norm[token,:]  (RelAttention.forward
 * transformer_code.py:136-160 + compute_pe mdl_vog.py:456-490 + do_cross
 * mdl_srl_utils.py:30-69 + Linear(5,H)+ReLU mdl_vog.py:446-451,580-585; the
 * [S,N,N,H] tensor is never materialised). use_rel=0 gives Attention.forward
 * (transformer_code.py:42-50). q, k, vt: fragment order of vog_qkv_proj (npad = N up
 * to 32). u: [n_vid, NP, H] fp32; token j of sequence s uses row
 * (s / seq_per_vid)*NP + (s % seq_per_vid)*n_box + (j % n_box).
 * out16: [S*N, H*dp] t16 row-major (heads concatenated, padded). */
#define VOG_LOGIT_WORDS 32     /* words of one logit_max report ... */
#define VOG_LOGIT_STRIDE 32    /* ... this many 32-bit words apart (one 128-byte line each) */
typedef struct vog_attn_args {
  const void* q; const void* k; const void* vt; void* out16;
  const float* u; const float* pe_b;
  int S, N, H, dp, npad; int use_rel; int n_box, seq_per_vid, NP;
  float inv_scale; vog_dtype dtype;
  /* optional: 4 device bytes owned by the caller. With it, bf16 sequences of >= 1024 tokens and head
   * dims <= 192 run attn_tile2_kernel (64 queries per wave, softmax against a fixed per-row reference
   * overlapped with the MFMAs; csrc/attn_tile2_dev.h); the flag is cleared, raised by the kernel if a
   * row left the safe range of that formulation, and a second (normally empty) launch of the
   * running-maximum kernel redoes the call when it was raised. NULL: running-maximum kernel only.
   * guard_precleared != 0: the caller guarantees *guard_flag == 0 on entry (vog_forward keeps the flags in the workspace
   * region its prologue zero-fills), so the clearing launch is skipped. */
  int* guard_flag;
  int guard_precleared;
  /* round 6, hi + lo operands (optional; both or neither): q_lo / k_lo = the 16-bit remainders t16(x - t16(x)) of the fp32 Q / K
   * projections, same fragment order as q / k (vog_qkv_args.q_lo / k_lo). With them Q.K^T = q.k + q_lo.k + q.k_lo (three MFMAs,
   * fp32 accumulate): the logits carry ~2^-21 relative operand error instead of 2^-11 (f16) - what a checkpoint with sharp
   * attention needs. Any sequence length (more than 256 tokens: the running-maximum tile kernel with the K
   * remainders in its LDS ring). out16_lo (optional): remainder of out16, same layout (read
   * by a hi + lo vog_tx_tail_fwd). logit_max (optional): VOG_LOGIT_WORDS device words VOG_LOGIT_STRIDE words apart (4 KiB),
   * which the launch only ever RAISES: zero them for a fresh measurement; the largest of them after the launch is the largest
   * |logit| (after bias and scale, in nats) seen since, as the bits of a non-negative float (the workgroups spread over the
   * words; a wave issues an atomic only when it would raise its word). */
  const void* q_lo; const void* k_lo; void* out16_lo; unsigned int* logit_max;
} vog_attn_args;
int vog_rel_attention_fwd(const vog_attn_args* a, void* stream);

/* Attention of mul_tx layer 0 through the token structure (exact): token (arg a, proposal p) =
 * [vis[p] || lang[a]], so k = Kv[p] + Kl[a], v = Vv[p] + Vl[a] and the bias depends on (p, p') only.
 * The logit of key (a', p') is X[p'] + Y[a'] with X = q.Kv[p'] + bias, Y = q.Kl[a']: the softmax over
 * the nsrl*nppf keys FACTORISES into softmax_p'(X) x softmax_a'(Y), and the output is
 *     softmax_p'(X) . Vv  +  softmax_a'(Y) . Vl
 * - nppf + nsrl keys per query instead of nsrl*nppf (25 instead of 100 at gt5, 405 instead of 2000
 * at p100), and no fanned-out K / V in HBM. q: [S,H,npad_q*dp] fragment order, N_q = nsrl*nppf
 * tokens (token = a*nppf + p); kv, vv: [S,H,npad_kv*dp] fragment order, nppf tokens; pl: the
 * language projection [n_lang*nsrl, 3*H*dp] fp32 of vog_qkv_args (K block at column H*dp, V block at
 * 2*H*dp); u / pe_b / seq_per_vid / NP as in vog_attn_args with n_box = nppf. out16: [S*N_q, H*dp]. */
typedef struct vog_attn_struct_args {
  const void* q; const void* kv; const void* vv; const float* pl; void* out16;
  const float* u; const float* pe_b;
  int S, H, dp, nsrl, nppf, npad_q, npad_kv, nfrm, lang_per_vid, nc_v;
  int use_rel, seq_per_vid, NP; float inv_scale; vog_dtype dtype;
  /* q_visual = 1: q holds only the nppf VISUAL query parts Qv ([S,H,npad_kv*dp], like kv) and the
   * kernel forms q(a, p) = Qv[p] + Ql[a] itself (Ql = pl columns [0, H*dp)): nothing is fanned out
   * in HBM (plain vog_qkv_proj over the visual rows, pl = NULL). npad_q is ignored. */
  int q_visual;
  /* round 5, optional: one int, zero at launch. With it, q_visual launches over several key blocks (p100) use the E x F
   * factorisation (141 instead of 330 us at cfg 4): the kernel sets it when a row may leave the safe range of its 16-bit
   * fragments and the same call then re-runs the per-row kernel (an empty launch otherwise). NULL: per-row kernels only. */
  int* guard_flag;
  /* round 6, hi + lo operands (optional; both or neither; q_visual form; any number of visual key blocks): the 16-bit remainders of Qv / Kv, same
   * fragment order; the language parts are split in the kernel from the fp32 `pl`. out16_lo / logit_max: as in vog_attn_args
   * (the logit bound is max|x| + max|y| of the separable parts). */
  const void* q_lo; const void* kv_lo; void* out16_lo; unsigned int* logit_max;
} vog_attn_struct_args;
int vog_rel_attention_struct_fwd(const vog_attn_struct_args* a, void* stream);

/* The launches behind the two attention entries (csrc/attention.hip): which kernel runs, and how, is decided by a pure host
 * function per entry that reads only the scalar fields of the argument block and whether its optional pointers (q_lo, k_lo /
 * kv_lo, out16_lo, guard_flag) are null. The enumerators are the kernel function names. */
typedef enum vog_attn_kernel {
  VOG_ATTN_GUARD_CLEAR_KERNEL = 0, VOG_ATTN_SB_KERNEL, VOG_ATTN_FRAG_LEAN_KERNEL, VOG_ATTN_FRAG8_KERNEL, VOG_ATTN_FRAG_KERNEL,
  VOG_ATTN_TILE_KERNEL, VOG_ATTN_TILE2_KERNEL, VOG_ATTN_STRUCT1_LEAN_KERNEL, VOG_ATTN_STRUCT1_DMA_KERNEL, VOG_ATTN_STRUCT_KERNEL,
  VOG_ATTN_STRUCT_LDS_KERNEL, VOG_ATTN_STRUCT_EF_KERNEL, VOG_ATTN_KERNELS
} vog_attn_kernel;
typedef enum vog_attn_guard {
  VOG_ATTN_GUARD_NONE = 0,   /* the kernel gets no guard word */
  VOG_ATTN_GUARD_FLAG = 1,   /* the launch writes the word: clears it, or raises it when a row left the safe range */
  VOG_ATTN_GUARD_GATE = 2    /* fallback pass: the launch does its work only if the word was raised */
} vog_attn_guard;
typedef struct vog_attn_launch {
  int kernel;                /* vog_attn_kernel */
  int flag;                  /* the SPLIT (0 / 1) or WPE template argument of kernels that have one, else 0 */
  unsigned int grid, block;  /* workgroups, threads per workgroup */
  unsigned int lds;          /* dynamic LDS bytes of the launch */
  unsigned int lds_cap;      /* the dynamic-LDS limit raised for the kernel before its first launch; 0 = none */
  int guard;                 /* vog_attn_guard */
} vog_attn_launch;
/* out: room for 3 (vog_attn_plan) / 2 (vog_attn_struct_plan) launches; *n = how many. Returns what the entry itself would
 * return for a shape it refuses (vog_last_error says why), 0 otherwise. No device call; pointers are only tested for null. */
int vog_attn_plan(const vog_attn_args* a, vog_attn_launch* out, int* n);
int vog_attn_struct_plan(const vog_attn_struct_args* a, vog_attn_launch* out, int* n);
const char* vog_attn_kernel_name(int kernel);   /* "attn_sb_kernel", ...; NULL outside the enum */
/* Whether the hi + lo plan of a shape succeeds (what vog_ctx_split_supported asks per attention step). */
int vog_attn_split_supported(int N, int dp);
int vog_attn_struct_split_supported(int nppf, int nsrl, int dp);

/* y = LayerNorm(x) * gamma + beta, eps 1e-5 (ResidualBlock.forward
 * transformer_code.py:30-31; the residual add is fused into the producing
 * GEMM's epilogue). x,y32: [rows,d] fp32; y16 optional t16 copy. */
int vog_residual_layernorm(const float* x, const float* gamma, const float* beta,
                           float* y32, void* y16, int rows, int d, vog_dtype dtype,
                           void* stream);

/* ---- fused encoder-layer tail ---------------------------------------------------------------
 * Everything of one (Rel)EncoderLayer after the attention is row-local, so ONE launch does
 *     x1 = LayerNorm(x + attn Wo^T)                    (RelMultiHead.forward tail transformer_code.py:184-186
 *                                                       + ResidualBlock.forward :30-31)
 *     y  = LayerNorm(x1 + W2 relu(W1 x1 + b1) + b2)    (FeedForward.forward :80-81 + ResidualBlock)
 * and, for the last mul_tx layer (score != NULL), the score head on top of it
 *     logit = lin2.2 . relu(lin2.0 y + b) + b          (mdl_vog.py:224-230,675-677)
 *     mdl_outs / mdl_outs_eval = inverse regroup + sigmoid * masks   (as vog_score_head)
 * for 64 token rows per workgroup: replaces vog_gemm_bias_act x 3, vog_residual_layernorm x 2
 * (+ the lin2 GEMM and vog_score_head) and all their intermediates in HBM.
 *   attn16  [M, kwo] t16 row-major = out16 of vog_rel_attention(_struct)_fwd (kwo = H*dp, kwo % 64 == 0)
 *   wo_p / w1_p / w2_p / wl_p: Wo_pad [d, kwo], linear1 [dh, d], linear2 [d, dh], lin2.0 [256, d] in
 *           the 32x16 fragment order of vog_pack_w_frag32 (types: dtype, dtype, dtype, head_dtype)
 *   residual [M, ldr] fp32, or res_vislang = the implicit vis||lang token matrix (exactly one of them)
 *   y32 / y16 (type y16_dtype, -1 = dtype): [M, d] outputs, either may be NULL
 *   x1_scratch: vog_tx_tail_scratch_bytes(M, d) bytes (0 for every supported width), workgroup-private spill slab
 * Shapes (vog_tx_tail_supported(d, dh, kwo) == 1): d in {256, 384, 512, 768}, dh = d/2, and per width
 *   d = 256: kwo in {256, 320, 384}        d = 384: kwo in {384, 512, 640}
 *   d = 512: kwo % 64 == 0, kwo <= 768     d = 768: kwo % 192 == 0, kwo <= 768
 * (kwo = heads x padded head width; 1 .. 8 heads of a 256- / 384-wide stack give the sets above, 7 heads aside). Other shapes
 * use the unfused entries; vog_tx_tail_fwd fails on them. The hi + lo operands below exist for d in {512, 768} only: with
 * remainder pointers at d = 256 / 384 the call fails without launching (and vog_ctx_split_supported is 0 for such a model). */
struct vog_score_args;
typedef struct vog_tx_tail_args {
  const void* attn16; int kwo;
  const void* wo_p; const void* w1_p; const void* w2_p;
  const float* residual; int64_t ldr;
  const struct vog_vislang_args* res_vislang;
  const float* ln1g; const float* ln1b; const float* b1; const float* b2; const float* ln2g; const float* ln2b;
  float* y32; void* y16; int y16_dtype;
  const void* wl_p; const float* bl;            /* score head (with `score`): lin2.0 packed / bias */
  const struct vog_score_args* score;            /* h1 is ignored; w2 / b2 = lin2.2 */
  int head_dtype;                                /* vog_dtype of wl_p (VOG_F16) */
  float* x1_scratch;
  int M, d, dh; vog_dtype dtype;
  /* round 6, hi + lo operands (optional; the first four together, not with `score`): attn16_lo = out16_lo of the attention,
   * w*_p_lo = the 32x16 fragment-ordered 16-bit remainders t16(w - t16(w)) of the fp32 weights. Every GEMM stage is then
   * W.X + W_lo.X + W.X_lo (three MFMAs, 32 rows per workgroup) and y16_lo (optional) receives the remainder of y16: the tail of a
   * layer whose OUTPUT feeds another attention layer of a checkpoint with sharp logits. */
  const void* attn16_lo; const void* wo_p_lo; const void* w1_p_lo; const void* w2_p_lo; void* y16_lo;
} vog_tx_tail_args;
int vog_tx_tail_supported(int d, int dh, int kwo);
int64_t vog_tx_tail_scratch_bytes(int M, int d);
int vog_tx_tail_fwd(const vog_tx_tail_args* a, void* stream);
/* One whole (Rel)EncoderLayer.forward (transformer_code.py:189-203 = RelMultiHead :176-186 + the two
 * ResidualBlocks :21-31 + FeedForward :73-81) as ONE entry - SURVEY.md 8(b)'s `vog_encoder_layer_fwd`:
 * QKV projection -> RelAttention -> tail, three launches, nothing but Q/K/V^T fragments and the 16-bit
 * attention rows in HBM between them. The three argument blocks are the ones of the stand-alone entries
 * and must be consistent (qkv.q/k/vt = attn.q/k/vt, attn.out16 = tail.attn16, tail.M = qkv.S * qkv.N,
 * tail.kwo = qkv.H * qkv.dp); the call checks that. */
typedef struct vog_encoder_layer_args {
  vog_qkv_args qkv;
  vog_attn_args attn;
  vog_tx_tail_args tail;
} vog_encoder_layer_args;
int vog_encoder_layer_fwd(const vog_encoder_layer_args* a, void* stream);

/* host: fp32 [N, ld] (first K columns) -> 16-bit 32x16 fragment order, N*K halfwords:
 * [N/32][K/16][lane = ((k%16)/8)*32 + n%32][k%8]  (N % 32 == 0, K % 16 == 0). */
int vog_pack_w_frag32(const float* w, int64_t ld, int N, int K, void* dst_host, vog_dtype dtype);

/* Proposal + segment encoders + their concat in ONE launch (prop_feats_encode / seg_feats_encode
 * mdl_vog.py:291-314, Linear+ReLU :202-207; concat_prop_seg_feats mdl_conc_single.py:51-66,156-174,
 * mdl_conc_sep.py:44-62): out[r, :prop_enc] = relu(W_p prop[r] + b_p), out[r, prop_enc:] =
 * relu(W_s seg[r / nppf0] + b_s). prop: [n_prop_rows, prop_dim] fp32, seg: [n_prop_rows/nppf0, seg_dim]
 * fp32 (read once, rounded to `dtype` in registers); w_*_f: weights in the fragment order of
 * vog_pack_w_frag, type `dtype`; c32 / c16 (type c16_dtype): [n_prop_rows, ldc], either may be NULL.
 * Needs feature dims % 256 == 0, encode sizes % 32 == 0 and <= 256 (vog_vis_encode_supported);
 * other shapes use vog_cast_f32_to_t16 + vog_gemm_bias_act (+ vog_splitk_finish). */
typedef struct vog_visenc_args {
  const float* prop; const float* seg;
  const void* w_prop_f; const void* w_seg_f; const float* b_prop; const float* b_seg;
  float* c32; void* c16; int64_t ldc; int c16_dtype;
  int n_prop_rows, nppf0, prop_dim, seg_dim, prop_enc, seg_enc; vog_dtype dtype;
  /* lean = 1: 64-row x 128-column workgroups (32 of them at cfg 2) that read the fp32 rows once per column
   * half and stage them in LDS: ~2x the latency of the wide form but ~5x less busy-CU time - the form used
   * when the encoders share the launch of a persistent BiLSTM layer (csrc/pair.hip). Same results up to
   * fp32 summation order. */
  int lean;
  /* Replication of the segment rows over the nppf0 proposals of their frame (lean form only). 0: done by
   * vog_vis_encode - inside the encoder kernel for nppf0 <= 16, otherwise by a copy kernel it launches
   * behind it (at 100 proposals per frame the 25 MB of replica stores took the 6 workgroups owning the
   * segment rows 100 us longer than everybody else). 1: vog_vis_encode writes replica 0 only and the caller
   * runs vog_seg_replicate (the forward does, so that the encoder kernel stays ONE launch and can share
   * the launch of a BiLSTM layer). */
  int defer_replicas;
  /* round 6, hi + lo operands (optional; all three or none; lean = 1; vog_seg_replicate copies c16_lo too): w_*_f_lo = the fragment-ordered 16-bit
   * remainders t16(w - t16(w)) of the fp32 weights; the fp32 feature rows are split the same way in the kernel and a k-step is
   * x.w + x_lo.w + x.w_lo (three MFMAs). c16_lo: the remainder of the output rows, laid out like c16 (read by a hi + lo
   * vog_qkv_proj). */
  const void* w_prop_f_lo; const void* w_seg_f_lo; void* c16_lo;
} vog_visenc_args;
int vog_vis_encode_supported(int prop_dim, int seg_dim, int prop_enc, int seg_enc);
int vog_vis_encode(const vog_visenc_args* a, void* stream);
/* rows r*nppf0 + j (j = 1 .. nppf0-1), columns [prop_enc, prop_enc + seg_enc) of c32 / c16 := row r*nppf0 */
int vog_seg_replicate(const vog_visenc_args* a, void* stream);

/* The concat alone, from encoder outputs computed elsewhere (vog_batch.enc_prop / enc_seg; the forward's `vis_concat` step):
 * out[r, :prop_enc] = enc_prop[r], out[r, prop_enc:] = enc_seg[r / nppf0], r < n_rows, written in the three forms the
 * transformers read: c32 fp32, c16 = t16(o) in c16_dtype, c16_lo = t16(o - f32(c16)) (the hi + lo plan's remainder rows) -
 * the roundings of vog_vis_encode's own epilogue, so the rows equal the encoders' bit for bit. Any of the three may be NULL
 * (c16_lo needs c16). enc_prop: [n_rows, prop_enc] fp32, enc_seg: [n_rows / nppf0, seg_enc] fp32; ldc >= prop_enc + seg_enc.
 * 16-byte accesses where both encode sizes and ldc are multiples of 8 (or 4) and the pointers are 16-byte aligned, one
 * element per thread otherwise. */
typedef struct vog_visconcat_args {
  const float* enc_prop; const float* enc_seg;
  float* c32; void* c16; void* c16_lo; int64_t ldc; int c16_dtype;
  int n_rows, nppf0, prop_enc, seg_enc;
} vog_visconcat_args;
int vog_vis_concat(const vog_visconcat_args* a, void* stream);

/* What a forward that starts behind obj_tx still needs next to the stack's fp32 output rows (vog_batch.obj_out; the forward's
 * `obj_restore` step): y16 = t16(x), y16_lo = t16(x - f32(y16)) for every row of x [n_rows, d_obj] fp32 - the roundings of
 * the encoder-layer tail's own epilogue (RNE cast, remainder from the exact fp32 difference), so the copies equal what the
 * last obj_tx layer would have written - and the segment columns [d_obj - seg_enc, d_obj) of prop_seg, each enc_seg row
 * [n_rows / nppf0, seg_enc] replicated to its nppf0 proposal rows (the sep head reads them there). x is dense; the three
 * outputs share the row pitch ldc >= d_obj, and nothing is written between a row's end and the next row. y16, y16_lo and
 * the (prop_seg, enc_seg) pair are optional (y16_lo needs y16). 16-byte accesses where d_obj, seg_enc and ldc are multiples
 * of 8 (or 4) and the pointers are 16-byte aligned, one element per thread otherwise. */
typedef struct vog_objrestore_args {
  const float* x; const float* enc_seg;
  void* y16; void* y16_lo; float* prop_seg; int64_t ldc; int y16_dtype;
  int n_rows, nppf0, d_obj, seg_enc;
} vog_objrestore_args;
int vog_obj_restore(const vog_objrestore_args* a, void* stream);

/* dst[i] = (t16) src[i] for two arrays in one launch (raw proposal / segment
 * features -> the encoders' MFMA operand type; replaces the implicit fp32 read
 * of nn.Linear in prop_feats_encode / seg_feats_encode mdl_vog.py:291-314).
 * n0, n1 multiples of 4; src1 may be NULL. */
int vog_cast_f32_to_t16(const float* src0, void* dst0, int64_t n0, const float* src1, void* dst1,
                        int64_t n1, vog_dtype dtype, void* stream);

/* u[v, r, h] = sum_c W_pe[h,c] * norm(box[v,r,c]), norm = x/vid_w, y/vid_h,
 * x/vid_w, y/vid_h, frame/nfrm_div (compute_pe mdl_vog.py:456-463).
 * props: [n_rows, 7] fp32 (pad_proposals). */
int vog_box_u(const float* props, const float* w_pe, float* u, int n_rows, int H,
              float vid_w, float vid_h, float nfrm_div, void* stream);

/* Token re-index (get_srl_arg_seq_to_sent_seq mdl_vog.py:67-95):
 * tok[b*T+t] = words[b, mask[b,t]] if mask[b,t] >= 0 else vocab_size. */
int vog_srl_gather(const int64_t* words_ind, const int64_t* word_mask, int32_t* tok,
                   int Bn, int T, int nsrl, int seq_len, int vocab_size, void* stream);
/* Packed-sequence schedule of the BiLSTM, as GEMM out_rows (pitch 4R, segment
 * width 4R): rows[dir*Bn*T + b*T + t] = dir*(T*Bn - 1) + step*Bn + b with step = t
 * (dir 0) or len_b-1-t (dir 1), so that row*4R + col lands in gxs[dir][step][b][:];
 * -1 for t >= len_b. */
int vog_lstm_schedule(const int64_t* lens, int32_t* rows, int Bn, int T, void* stream);

/* Fused prologue of the language path (one launch instead of memset + vog_srl_gather +
 * vog_lstm_schedule): zero `zero_bytes` at `zero` (multiple of 16), fill the `ones_bytes` (multiple of
 * 16) that follow them with 0xff (the "not written yet" pattern of the persistent BiLSTM's hand-off
 * slots), token re-index and the packed-sequence schedule. */
int vog_lang_prep(void* zero, int64_t zero_bytes, int64_t ones_bytes, const int64_t* words_ind, const int64_t* word_mask,
                  const int64_t* lens, int32_t* tok, int32_t* rows, int Bn, int T, int nsrl,
                  int seq_len, int vocab_size,
                  /* optional (a0_frag != NULL): also gather the tokens' 16-bit embedding rows
                   * [vocab+1, emb_dim] into a0_frag in the A-fragment order of vog_gemm_args.a_frag
                   * (rows beyond Bn*T of the last 16-row tile must already be zero) */
                  const void* emb16, void* a0_frag, int emb_dim, void* stream);

/* Fused prologue of the visual path (one launch instead of vog_cast_f32_to_t16 + up to two
 * vog_box_u): u0/u1 = bias precursors for obj_tx / mul_tx (either w_pe may be NULL). */
typedef struct vog_visprep_args {
  const float* src0; void* dst0; int64_t n0; const float* src1; void* dst1; int64_t n1; vog_dtype dtype;
  const float* props; int n_rows; float vid_w, vid_h;
  const float* w_pe0; float* u0; int H0; float nfrm_div0;
  const float* w_pe1; float* u1; int H1; float nfrm_div1;
} vog_visprep_args;
int vog_vis_prep(const vog_visprep_args* a, void* stream);
/* vog_lang_prep + vog_vis_prep in ONE launch (the two prologues are independent of each other;
 * one launch less on the forward's dependent chain). Arguments as for the two entries. */
int vog_prep_fused(void* zero, int64_t zero_bytes, int64_t ones_bytes, const int64_t* words_ind, const int64_t* word_mask,
                   const int64_t* lens, int32_t* tok, int32_t* rows, int Bn, int T, int nsrl,
                   int seq_len, int vocab_size, const void* emb16, void* a0_frag, int emb_dim,
                   const vog_visprep_args* vis, void* stream);

/* One time step of one BiLSTM layer, both directions, packed-sequence
 * semantics (LSTMEncoder.forward mdl_srl_utils.py:134-148; nn.LSTM gate order
 * i,f,g,o). gxs: [2][T][Bn][4R] fp32 = x W_ih^T + b_ih + b_hh in (direction, step)
 * order (vog_lstm_schedule + the GEMM's out_rows scatter); whh: the 16-bit
 * recurrent weights in MFMA-fragment order as packed by vog_lstm_pack_whh;
 * h_in/h_out: [Bn16, 2R] t16 ping-pong state; c: [Bn16,2R] fp32; out16:
 * [Bn*T, 2R] t16 (zero where t >= len). */
typedef struct vog_lstm_step_args {
  const float* gx; const void* whh; const void* h_in; void* h_out; float* c;
  void* out16; const int64_t* lens; int Bn, T, R, step; vog_dtype dtype;
  /* out_frag = 1: out16 is written in the A-fragment order of vog_gemm_args.a_frag
   * (K = 2R, rows m = b*T + pos) and every active step also writes h into row
   * final_row0 + b (the final hidden state ends up there). 0: row-major [.., 2R]. */
  int out_frag; int final_row0;
} vog_lstm_step_args;
int vog_bilstm_step(const vog_lstm_step_args* a, void* stream);
/* ALL T steps of one BiLSTM layer in ONE launch (persistent workgroups): 2 x R/32 workgroups of 8 waves,
 * every wave keeps its 16 rows of W_hh in registers for the whole sequence (W_hh is read once per
 * layer instead of once per step). Between steps the hidden state goes through `hx` =
 * [T slots][2 dirs][Bn][R] 16-bit values, one slot per step, which must hold 0xffff in every halfword
 * at launch (vog_lang_prep / vog_prep_fused `ones_bytes` arm it; vog_bilstm_hx_bytes gives the size):
 * every value validates itself - 0xffff is a NaN pattern no h can take - so a consumer needs no tag,
 * flag or fence, just one (re-tried) 16-byte L1-bypassing load per thread and step; the workgroup
 * stages the vector in LDS (double buffered) and every wave reads its MFMA B fragments from there.
 * Publishing: if all workgroups of a direction run on ONE XCD (they report their XCC id in `sync` at
 * start; small layers) every lane stores its value with a store that stays in that XCD's L2; otherwise
 * the workgroup's 64 bytes per sentence are written through by one wave (0.75 / 1.33 us per exchange,
 * scratch/ubench/handoff_v3.hip). Measured (cfg 2, Bn = 4, R = 1024): 2.5 us per step (3.0 in round 2).
 * Requires Bn <= 16 and R/32 in {1,2,4,32} (vog_bilstm_layer_supported); sync (256 x u32) must be zero
 * at launch (vog_lang_prep does it); every wait is bounded (~1 s): on timeout sync[2] is set, the
 * kernel drains and writes NaN into ALL its output rows so that a stalled run cannot pass for a result.
 * CO-RESIDENCY: all 2 x R/32 workgroups (one per CU) must be resident at once; launch at most 4
 * instances concurrently on a 256-CU part (HIP's 4 hardware queues guarantee that for streams).
 * LIMITS: vog_bilstm_layer takes 1 .. 16 sentences (one 16-column MFMA tile per wave), all three input forms.
 * vog_bilstm_layer_wide takes 17 .. 32 (two column tiles per wave on the same W_hh registers; same argument struct, same
 * hx / sync / fault / poison contract, hx = vog_bilstm_hx_bytes(Bn, T, R)): the gxs form and the gate table (Bn * T <= 768
 * staged token ids), not the in-kernel projection (wih != NULL is refused: it reaches 80 columns), T * Bn * R <= 2^26. Per
 * sentence it performs the arithmetic of vog_bilstm_layer operation for operation: one wide launch returns the bits of two
 * narrow launches over sentences [0, 16) and [16, Bn) (tests/test_gpu_lstm_wide.py). It uses up to 140,304 B of LDS
 * (R = 1024, Bn = 32: two staging buffers; Bn > 32 would not fit 160 KB) and is never part of a pair launch.
 * The wide form keeps the grid of 2 x R/32 workgroups - ONE team per launch - so the co-residency note above and the count
 * of four concurrent instances hold for it unchanged. Several independent 64-workgroup teams in one launch would not:
 * workgroups are dealt round-robin to the XCDs, one XCD can fill with slices of teams that are incomplete on another, and
 * every team then waits out its time-out. */
typedef struct vog_lstm_layer_args {
  const float* gxs; const void* whh; void* hx; uint32_t* sync; void* out16;
  const int64_t* lens; int Bn, T, R; vog_dtype dtype;
  int out_frag;   /* 1: out16 in the A-fragment order of vog_gemm_args.a_frag (as vog_bilstm_step) */
  /* Fused input projection (wih != NULL; gxs is then ignored): the kernel computes x W_ih^T + bias for
   * its own gate rows in a prologue (W_ih streamed once through registers, the layer input staged in
   * LDS) - no separate GEMM launch and no [2][T][Bn][4R] fp32 round trip. wih: vog_lstm_pack_w of
   * (weight_ih, weight_ih_reverse) [2][4R][K]; xa: layer input [Bn*T (row b*T + t), K] t16 in the
   * A-fragment order of vog_gemm_args.a_frag (pad rows of the last 16-row tile readable); bias: [2][4R]
   * fp32 = b_ih + b_hh per direction. Needs Bn*T <= vog_bilstm_fused_cols() (80: a bs = 4 batch with 20-word sentences) and
   * K % 256 == 0. */
  const void* wih; const void* xa; const float* bias; int K;
  /* round 5: sticky fault counter (optional; device memory or device-visible pinned host memory): +1 per launch whose
   * hand-off timed out. The library never clears it (sync[2] is re-zeroed by the next forward's prologue): the host reads
   * it when it looks at the results - a stalled forward is an ERROR at the API, not NaN scores with rc 0 (the reference's
   * LSTM, utils/mdl_srl_utils.py:114-169, cannot fail by scheduling). inject_stall: test hook, 1 = the launch behaves as
   * if its hand-off had timed out at once, 2 = only the workgroups of direction 1 do. Whichever workgroup ends dead first
   * reports (sync[3], re-armed by the prologue): exactly +1 per stalled launch. */
  uint32_t* fault; int inject_stall;
  /* round 6, gate table (gx_table != NULL; gxs and wih are then ignored): the layer's input is an embedding row, so its
   * projection depends on the TOKEN alone. gx_table = [vocab + 1][2][R][4] fp32, row v = emb[v] W_ih^T + b_ih + b_hh for
   * (direction, unit, gate i f g o) - built once per checkpoint for the whole vocabulary (vog_ctx_finalize; 164 MB at vocab 5000,
   * R = 1024); tok = [Bn * T] token ids (vog_lang_prep). The kernel reads its gate inputs of step s + 1 from the rows of
   * that step's tokens while step s runs: no input projection for this layer, neither as a GEMM launch nor in the kernel's
   * prologue, for any Bn * T (LSTMEncoder.forward, utils/mdl_srl_utils.py:134-148). */
  const float* gx_table; const int32_t* tok;
} vog_lstm_layer_args;
int vog_bilstm_layer_supported(int Bn, int R);
int vog_bilstm_fused_cols(void);                      /* largest Bn*T the in-kernel input projection (wih) takes: 80 */
int64_t vog_bilstm_hx_bytes(int Bn, int T, int R);   /* size of vog_lstm_layer_args.hx */
int vog_bilstm_layer(const vog_lstm_layer_args* a, void* stream);
int vog_bilstm_layer_wide_supported(int Bn, int R);  /* 1 for 17 <= Bn <= 32 and an R vog_bilstm_layer_supported takes */
int vog_bilstm_layer_wide(const vog_lstm_layer_args* a, void* stream);

/* host: [2][4R][R] fp32 (weight_hh_l*, weight_hh_l*_reverse) -> fragment order, 16 bit.
 * dst holds 2*4R*R halfwords: [dir][unit/4][k/32][lane 64][8]. */
int vog_lstm_pack_whh(const float* whh_fwd, const float* whh_bwd, void* dst_host, int R, vog_dtype dtype);
/* same packing for a [4R][K] pair (weight_ih): [dir][unit/4][K/32][lane 64][8], K % 32 == 0 */
int vog_lstm_pack_w(const float* w_fwd, const float* w_bwd, void* dst_host, int R, int K, vog_dtype dtype);

/* lang[b,a,:] = relu(W [full[b,cap0] || full[b,cap1]] + bias) * msk
 * (retrieve_srl_arg_from_lang_encode mdl_vog.py:97-140). full: [Bn*T, L] fp32. */
int vog_srl_argvec(const float* full, const int64_t* capture, const int64_t* inds_msk,
                   const float* w, const float* bias, float* lang,
                   int Bn, int T, int nsrl, int L, void* stream);

/* Build the mul_tx token matrix (concate_vis_lang_feats mdl_vog.py:316-344 +
 * the regroup of conc_encode2 mdl_vog.py:693-699): row (s=(v,f), j=a*nppf+p) =
 * [vis[v, f*nppf+p, :dv] || lang[lv(v), a, :dl]]; writes fp32 and t16 copies. */
typedef struct vog_vislang_args {
  const float* vis; const float* lang; float* x32; void* x16;
  int n_vid, nfrm, nppf, nsrl, dv, dl; int lang_per_vid; /* 1: lang row = v, 0: v / nc_v */
  int nc_v; vog_dtype dtype;
} vog_vislang_args;
int vog_vislang_layout(const vog_vislang_args* a, void* stream);

/* lin2 second layer + inverse regroup + masks (mdl_vog.py:675-677, 724-737;
 * mdl_conc_single.py:118-122): logit = w2.h1[row] + b2 scattered to
 * mdl_outs[v, a, f*nppf+p]; eval = sigmoid * arg_msk * cmp_msk. */
typedef struct vog_score_args {
  const float* h1; const float* w2; const float* b2;
  const int64_t* arg_msk; const int64_t* cmp_msk;
  float* outs; float* outs_eval;
  int n_vid, nfrm, nppf, nsrl, dh; int conc_type; int ncmp, nc_v, nvl, nfrm0, nppf0;
} vog_score_args;
int vog_score_head(const vog_score_args* a, void* stream);

/* pred_cmp head of SEP (get_seg_verb_feats_to_process / compute_seg_verb_feats_out
 * mdl_vog.py:365-397, compute_fin_scores mdl_conc_sep.py:64-129). */
typedef struct vog_predcmp_args {
  const float* final_hidden;   /* [B*nvl, L] fp32 */
  const float* prop_seg;       /* [B*ncmp, NP, dps] fp32; seg part = cols [dp0, dps) */
  const float* w0; const float* b0; const float* w2; const float* b2;
  const float* outs;           /* mdl_outs [B, ncmp, nsrl, NP] */
  const int64_t* arg_msk; const int64_t* cmp_msk; const int64_t* verb_ind;
  float* vidf_outs; float* fin_scores_loss; float* fin_scores;
  int B, ncmp, nvl, nsrl, NP, nfrm0, nppf0, L, dp0, dps;
} vog_predcmp_args;
int vog_pred_cmp_head(const vog_predcmp_args* a, void* stream);

/* Evaluator*.get_out_results_boxes (eval_vsrl_corr.py:162-220,289-345,357-424):
 * per (query,arg,video,frame) max/argmax over the frame's proposals, gather the
 * 7-d proposal row, pred_cmp index. Output is ONE packed record per query (the
 * unit of the cross-rank all-gather that replaces the pickle-file gather of
 * eval_vsrl_corr.py:125-140):
 *   float boxes[nsrl][ncmp][nfrm0][7]; float scores[nsrl][ncmp][nfrm0];
 *   int64 indexs[nsrl][nfrm0]  (temp: zeros; the reference returns float zeros) */
typedef struct vog_pred_args {
  const float* outs_eval; const float* props; const float* fin_scores; void* rec;
  int B, ncmp, nsrl, nfrm0, nppf0; int conc_type;
  /* round 6, optional: logit_max = the forward's [2 stacks][4 layers] reports of vog_attn_args.logit_max (4 KiB each); the head (the last
   * kernel of a forward) folds them into stats[0] (obj_tx) / stats[1] (mul_tx) with a system-scope atomic max - pinned host
   * memory, read by the host without a device synchronisation (vog_batch.stats). */
  const unsigned int* logit_max; unsigned int* stats;
  unsigned int* published;     /* 2 device words, zero at first use: what this caller's forwards last folded into `stats` (the host
                                * word is only touched when the value rises) */
} vog_pred_args;
int64_t vog_pred_record_bytes(int ncmp, int nsrl, int nfrm0);
int vog_pred_head(const vog_pred_args* a, void* stream);

/* Grounding metrics of B prediction records (GroundEval_SEP / _TEMP / _SPAT.eval_one_sent_idx, eval_fn_corr.py; reference
 * code/eval_fn_corr.py:302-747): per record the counts the host path derives from the unpickled record, as ONE packed word.
 * One launch for the whole batch, one wave per record; no atomics, no state between records or launches, no allocation, no
 * synchronisation. "First record of a sentence wins" and all averaging stay on the host.
 *
 * Annotation table (device arrays, int32; built on the host from a GroundEval_* instance, uploaded once):
 *   per sentence row s of the SRL csv [n_sent]: verb_id (index of lemma_verb in first-seen order; host aggregation only),
 *     in_split (1 = row of the validation split; host aggregation only), box_off / box_cnt = the boxes of the sentence's
 *     segment in gt_box[n_box][4] (x1 y1 x2 y2, the annotated integers) and gt_frm[n_box] (frame of each box, < nfrm0), in
 *     file order; arg_off / arg_cnt = the sentence's arguments in has_box[n_arg], ind_off[n_arg], ind_cnt[n_arg], in
 *     req_cls_pats_mask order; n_ground = groundable arguments (has_box == 1) of the WHOLE list, <= 15: arguments past the
 *     record's nsrl still count in `tot`;
 *   per argument: ind_off / ind_cnt = its entries of ind[n_ind], indices into the segment's boxes (0 <= ind < box_cnt[s]).
 *   nfrm0: the frame count the frame indices were checked against; must equal vog_gmetric_args.nfrm0.
 *
 * Rules (an argument is scored when has_box == 1 and its position is < nsrl; hit(arg, video, box) = IoU(predicted box of
 * (arg, video, frame of the box), annotated box) > 0.5 and score > prob_thresh; the IoU is float32, operation for operation
 * utils/box_utils.py:25-52 without fused multiply-add and with an IEEE division (0/0 = NaN = no hit), annotated integers
 * converted to float32; the float32 score is compared as a double against prob_thresh):
 *   sep   query_vid = the most frequent entry of indexs[nsrl][nfrm0] (first seen on ties). Correct iff query_vid == targ
 *         and some annotated box of the argument is hit in video query_vid. cons = 1, vidf = (query_vid == targ).
 *   temp  over the videos with cmp_msk == 1: the target video needs a hit; any other video v "fires" when a frame of
 *         sentence idx_verbs[v]'s segment (file order, duplicates included) is scored above the threshold, with the score of
 *         the FIRST such frame. Correct iff no video fired and the target (if unmasked) is hit. Decision: targ if correct,
 *         -1 if nothing fired, else the fired video with the highest score (first on ties). cons = all decisions equal and
 *         >= 0, vidf = cons and decision == targ.
 *   spat  per frame f, v = indexs[arg][f]: where the argument has annotated boxes in f, v == targ and a hit against one of
 *         them (x1, x2 of the annotated box + 720 * targ, added as integers); elsewhere NOT (v != targ and score above the
 *         threshold), and the frame is "free". Correct iff every frame behaves. Decision: targ if correct, -5 without free
 *         frames, else minus the frame number of the highest-scored free frame (first on ties; frame 0 gives 0).
 *         cons = all decisions equal, vidf = all decisions == targ.
 * result[b]: bits 0-3 res (correct arguments), 4-7 tot (= n_ground; 0 = not scored, the host path's None), 8 cons, 9 vidf,
 *   10 strict (res == tot); the host multiplies cons / vidf / strict by tot. Error bits, with the count bits zero:
 *   16 idx_verbs[b, targ_cmp[b]] != idx_sent[b]; 17 spat chose a video with cmp_msk != 1; 18 an index out of range
 *   (sentence row or idx_verbs entry outside [0, n_sent), targ_cmp or an entry of indexs read as a video outside [0, ncmp)).
 *   The kernel reads nothing through an out-of-range index. */
typedef struct vog_gmetric_table {
  const int32_t *verb_id, *in_split, *box_off, *box_cnt, *arg_off, *arg_cnt, *n_ground;   /* [n_sent] */
  const int32_t *gt_box, *gt_frm;                                                           /* [n_box][4], [n_box] */
  const int32_t *has_box, *ind_off, *ind_cnt;                                               /* [n_arg] */
  const int32_t *ind;                                                                       /* [n_ind] */
  int n_sent, n_box, n_arg, n_ind, nfrm0;
} vog_gmetric_table;
struct vog_val_log_args;
typedef struct vog_gmetric_args {
  const void* rec;            /* [B] records, layout of vog_pred_head, vog_pred_record_bytes(ncmp, nsrl, nfrm0) apart */
  const int64_t *idx_sent, *idx_verbs, *cmp_msk, *targ_cmp;   /* [B], [B,ncmp], [B,ncmp], [B] (device) */
  const vog_gmetric_table* tab;                               /* host struct of device pointers */
  int32_t* result;            /* [B] packed per-query result */
  int B, ncmp, nsrl, nfrm0, conc_type; double prob_thresh;
  /* Optional: the validation log of this step written by the SAME launch (see vog_val_log below; log->B == B): the result
   * words go into row *log->step of log->word_log as well (log->word_src is not read), extra blocks copy log's loss and
   * record pairs into their rows and set the marker. What vog_val_log(log) behind this call would do, one launch less;
   * `result` is written either way, and a step outside [0, rows) writes no row and sets log->bad_step. */
  const struct vog_val_log_args* log;
} vog_gmetric_args;
int vog_ground_metrics(const vog_gmetric_args* a, void* stream);
/* out[i] = IoU(a[i], b[i]) of n x1y1x2y2 box pairs with exactly the arithmetic of vog_ground_metrics (test entry). */
int vog_box_iou_f32(const float* a, const float* b, float* out, int n, void* stream);

/* SPAT / TEMP batch assembly on the device (verb_item_getter_SPAT / _TEMP,
 * code/dat_loader_simple.py:1046-1338): per-video items of B queries ([B, ncmp, ...], what
 * AV_CS.itemcollector stacks) -> the tensors the forward and the loss read, written straight into the
 * caller's (slot's) input buffers. Forward part (always): props [B,ncmp,NPv,7] -> [B,ncmp*NPv,7]
 * (spat: x1,x2 += vid_w*video, (frame,video,prop) order; temp: frame += nfrm0*video), region features
 * [.., prop_dim] and pnt mask (bytes, optional) re-ordered the same way, seg_feature_for_frms
 * [B,ncmp,nfrm0,seg_dim] -> [B,ncmp*nfrm0,seg_dim] (spat: (frame,video) order). Loss part (gt_in != NULL):
 * gt boxes [B,ncmp,G,5] shifted the same way, first num_box[b,v] of every video concatenated and zero
 * padded -> [B,G,5]; srl_boxes += boxes in front of target_cmp where srl_boxes_lens > 0; frm_mask
 * [B,ncmp*NPv,G] bytes = frame(prop) != frame(gt) for g < total boxes else 1; num_box_out [B] int64.
 * Bit-exact with the reference (fp32 adds, copies). */
typedef struct vog_assemble_args {
  const float* props_in; float* props_out; const float* region_in; float* region_out;
  const float* seg_in; float* seg_out; const unsigned char* pnt_in; unsigned char* pnt_out;
  const float* gt_in; float* gt_out; const int64_t* num_box; int64_t* num_box_out; const int64_t* target_cmp;
  const int64_t* srl_boxes_in; int64_t* srl_boxes_out; const int64_t* srl_boxes_lens; unsigned char* frm_out;
  int B, ncmp, nfrm0, nppf0, prop_dim, seg_dim, G, nv, nsrl, nbox, conc_type; float vid_w;
} vog_assemble_args;
int vog_assemble_batch(const vog_assemble_args* a, void* stream);

/* The same assembly from a FEATURE BANK in device memory: the per-video items of the whole dataset live in caller-owned
 * device tables of V rows, and a batch arrives as `index` [B, ncmp] int32 (device memory or pinned host memory, like the
 * *_in pointers above) - a few hundred bytes instead of 2 MB per query. region / seg are stored in `feat_dtype`:
 * VOG_BANK_F32, or VOG_F16 (half the footprint; rows are decoded to the fp32 rows the forward reads - exact - and the
 * 16-bit plans round every feature to f16 before any use, so nothing is lost there). Filling an f16 bank is
 * vog_cast_f32_to_t16 into its rows. pnt / gt / num_box are optional (NULL: the matching output must be NULL too).
 * Outputs and semantics are those of vog_assemble_batch, bit for bit, for VOG_CONC_SPAT / _TEMP; VOG_CONC_SEP is the plain
 * gather to [B, ncmp, ...] (no shift, no re-order; gt_out [B,ncmp,G,5], num_box_out [B,ncmp], pnt_out [B,ncmp,NPv]; the
 * srl_boxes members are not used). SEP frm_out (optional, with gt_out; needs bank.pnt): [B,ncmp,NPv,G] bytes, per video as the
 * reference loader pads it (code/dat_loader_simple.py:405-416, get_frm_mask :237-255): frame(proposal r) != frame(gt box g)
 * for r < the video's real proposals and g < num_box, 1 everywhere else (rows of padded proposals included). The real
 * proposals of a video end behind the last nonzero byte of its pnt row (padded rows are zero there).
 * An index outside [0, V) never forms an address: its rows are written as zeros (a video without boxes) and 1 is stored
 * to the sticky word `bad_index` (optional; pinned host memory lets the host poll it, as vog_batch.fault). */
#define VOG_BANK_F32 2
typedef struct vog_feature_bank {
  const void* region;            /* [V, nfrm0*nppf0, prop_dim] feat_dtype */
  const void* seg;               /* [V, nfrm0, seg_dim]        feat_dtype */
  const float* props;            /* [V, nfrm0*nppf0, 7] */
  const unsigned char* pnt;      /* [V, nfrm0*nppf0]  (optional) */
  const float* gt;               /* [V, G, 5]         (optional) */
  const int64_t* num_box;        /* [V]               (optional, with gt) */
  int64_t V;
  int feat_dtype;                /* VOG_BANK_F32 | VOG_F16 */
} vog_feature_bank;
typedef struct vog_bank_assemble_args {
  vog_feature_bank bank;
  const int32_t* index;          /* [B, ncmp] rows of the bank */
  float* props_out; float* region_out; float* seg_out; unsigned char* pnt_out;
  float* gt_out; int64_t* num_box_out; const int64_t* target_cmp;
  const int64_t* srl_boxes_in; int64_t* srl_boxes_out; const int64_t* srl_boxes_lens; unsigned char* frm_out;
  uint32_t* bad_index;
  int B, ncmp, nfrm0, nppf0, prop_dim, seg_dim, G, nv, nsrl, nbox, conc_type; float vid_w;
} vog_bank_assemble_args;
int vog_assemble_from_bank(const vog_bank_assemble_args* a, void* stream);

/* Byte ranges src -> dst in ONE launch (16-byte aligned pointers, any length, <= VOG_MAX_COPY_SEGS ranges). The sources may be
 * pinned host memory (hipHostMalloc / torch pin_memory: mapped into the device's address space): the kernel then reads over the
 * host link - the reference's `batch[k].to(device)` of the small per-batch arrays (code/utils/trn_utils.py:478, :562) without
 * one DMA transfer, and one transfer's fixed latency, per array. vog_assemble_batch accepts pinned-host *_in pointers the same way. */
#define VOG_MAX_COPY_SEGS 24
typedef struct vog_copy_seg { const void* src; void* dst; size_t bytes; } vog_copy_seg;
int vog_copy_segments(const vog_copy_seg* segs, int n, void* stream);

/* QUERY BANK gather: rows of several caller-owned device tables of Q rows each, named by ONE index [B], in one launch - the
 * per-query part of a batch (language arrays, masks, target_cmp, srl_boxes, metric columns: 18 to 21 keys of 8 bytes to a few
 * KB per query) without a host copy per key. For a key with per_batch == 0: dst[b * row_bytes ...] = table[index[b] *
 * row_bytes ...] for every b < B. A key with per_batch == 1 is one plain range of row_bytes bytes copied as it is (the index
 * is not used): the step number of a validation step, and any key the caller still stages, ride in the same launch. The key
 * table travels in the kernel's arguments, so the launch can be captured. Accesses are 16 bytes wide where table, dst and
 * row_bytes are all multiples of 16, otherwise the widest of 8, 4 or 1 bytes that all three share; tables, destinations and
 * sources of per-batch keys may be pinned host memory, like `index`. A row number outside [0, Q) never forms an address: its
 * destination rows are written as zeros and 1 is stored to the sticky word `bad_index` (optional; pinned host memory lets the
 * host poll it) - the feature bank's rule. Plain vector loads and stores, no atomics. */
#define VOG_MAX_GATHER_KEYS 32
typedef struct vog_gather_key {
  const void* table; void* dst; int64_t row_bytes; int per_batch;
} vog_gather_key;
typedef struct vog_gather_args {
  const int32_t* index;       /* [B] rows; device memory or pinned host memory */
  int B; int64_t Q; int n_keys;
  vog_gather_key keys[VOG_MAX_GATHER_KEYS];
  uint32_t* bad_index;        /* optional sticky word, pinned host allowed */
} vog_gather_args;
int vog_gather_rows(const vog_gather_args* a, void* stream);

/* Loss of one batch on the device: LossB_TEMP / LossB_SPAT
 * (code/mdl_conc_single.py:180-433) and LossB_SEP (code/mdl_conc_sep.py:220-447) with the IoU targets of
 * utils/box_utils.py:61-118: target[b,v,a,r] = max_k(IoU(prop r, gt box srl_boxes[b,v,a,k]) * mask *
 * [video(r) == target_cmp[b]] * srl_boxes_lens[b,v,a,k]) > 0.5; masked mean of BCE-with-logits over
 * mdl_outs, times the number of proposals, times loss_lambda. sep also returns the verb loss.
 *   mdl_outs [B, (ncmp if sep else 1), nsrl, NP]; NP = proposals per row block (temp / spat: all ncmp videos)
 *   pad_proposals [B,(ncmp,)NP,7], pad_gt_bboxs [B,(ncmp,)G,5] fp32; pad_frm_mask [B,(ncmp,)NP,G],
 *   pad_pnt_mask [B,(ncmp,)NP] bytes (nonzero = the IoU counts); srl_boxes / srl_boxes_lens
 *   [B,nv,nsrl,nbox], srl_arg_boxes_mask [B,nv,nsrl], target_cmp [B], num_cmp_msk [B,ncmp],
 *   verb_cmp [B,ncmp], verb_cross_cmp_msk [B,ncmp,ncmp] int64.
 *   out: 6 floats = loss, mdl_out_loss, verb_loss (0 unless sep), number of elements in the mean, 1 if the
 *   mean is the masked one (0: no argument has boxes -> plain mean), rows in the verb-loss mean.
 *   scratch: vog_loss_scratch_bytes(). Deterministic (fixed-order reduction, no atomics).
 * vog_loss_bwd: d loss / d mdl_outs [same shape] = (sigmoid(x) - target) [* video mask for sep] * NP * lambda / n
 *   for the elements in the mean, 0 elsewhere, and (optional, sep) d verb_loss / d vidf_outs [B, ncmp]; call after
 *   vog_loss_fwd with the same args (it reads out[3..5]). First link of the training path. */
typedef struct vog_loss_args {
  const float* mdl_outs; const float* vidf_outs;
  const float* pad_proposals; const float* pad_gt_bboxs;
  const unsigned char* pad_frm_mask; const unsigned char* pad_pnt_mask;
  const int64_t* srl_boxes; const int64_t* srl_boxes_lens; const int64_t* srl_arg_boxes_mask;
  const int64_t* target_cmp; const int64_t* num_cmp_msk; const int64_t* verb_cmp; const int64_t* verb_cross_cmp_msk;
  float* out; float* scratch;
  int B, ncmp, nv, nsrl, nbox, NP, G, nppf0, conc_type; float loss_lambda;
} vog_loss_args;
int64_t vog_loss_scratch_bytes(const vog_loss_args* a);
int vog_loss_fwd(const vog_loss_args* a, void* stream);
int vog_loss_bwd(const vog_loss_args* a, float* grad_mdl_outs, float* grad_vidf_outs, void* stream);

/* Validation log (csrc/val.hip): the results of ONE validation step -> row `step` of caller-owned device logs, so that a
 * whole validation loop is read back once, behind it. `step` is a word in device memory (pinned host memory works too): its
 * CONTENTS choose the row, so the launch can sit in a captured graph whose arguments are fixed addresses (a fed graph copies
 * the word from its staging buffer with the batch). Three source / log pairs, each optional (both NULL):
 *   loss_src  6 floats (vog_loss_args.out)                 -> loss_log [rows, 6]
 *   word_src  B result words (vog_gmetric_args.result)     -> word_log [rows, B]
 *   rec_src   B records of rec_words floats (vog_batch.pred_rec, rec_words = vog_pred_record_bytes / 4)
 *                                                          -> rec_log  [rows, B * rec_words]
 * and written[step] = 1 (optional, [rows] int32): the host tells a step that never ran from a zero loss. A launch writes its
 * own row only - no atomics, no state between launches; 16-byte accesses wherever a source and its row share their alignment.
 * A step outside [0, rows) never forms an address: nothing is written and 1 is stored to the sticky word `bad_step`
 * (optional; pinned host memory lets the host poll it, as vog_batch.fault). All pointers 4-byte aligned. */
typedef struct vog_val_log_args {
  const int32_t* step;
  const float* loss_src; float* loss_log;
  const int32_t* word_src; int32_t* word_log;
  const float* rec_src; float* rec_log;
  int32_t* written;
  uint32_t* bad_step;
  int rows, B, rec_words;
} vog_val_log_args;
int vog_val_log(const vog_val_log_args* a, void* stream);

/* SURVEY.md 8(f)-4, first slice of the backward: from d loss / d mdl_outs (vog_loss_bwd) through the score
 * head (lin2.0 -> ReLU -> lin2.2, code/mdl_vog.py:224-230, 675-677) and the tail of the LAST mul_tx encoder
 * layer (Wo + residual + LayerNorm + FFN + residual + LayerNorm, code/transformer_code.py:21-31, 73-81,
 * 189-203) to the gradients of every parameter on that path and of the tail's two inputs. fp32 on the
 * fp32 matrix pipe; the forward tail keeps nothing, so the activations are recomputed from `attn` and `x`.
 * All pointers are device fp32. attn: [M, d] the concatenated heads (input of Wo); x: [M, d] the layer
 * input (residual); rows m = (sequence s = (video, frame), token j = arg*nppf + p), M = n_vid*nfrm*nsrl*nppf;
 * d_mdl_outs: [n_vid, nsrl, nfrm*nppf] as vog_loss_bwd writes it. Weights in the reference's own shapes
 * (wo [d,d], w1 [dh,d], w2 [d,dh], wl = lin2.0.weight [dhead,d], wl2 = lin2.2.weight [dhead]); g_*: the
 * gradients, same shapes (g_bl2: 1 value; any g_* may be NULL = frozen, its GEMM / column sum is skipped);
 * d_attn / d_x: [M, d] or NULL. Pinned against autograd through
 * the reference modules (tests/golden/bwd__*.npz, oracle/make_golden_bwd.py). */
typedef struct vog_tail_bwd_args {
  const float* attn; const float* x; const float* d_mdl_outs;
  float* d_attn; float* d_x;
  const float *wo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b, *wl, *bl, *wl2;
  float *g_wo, *g_ln1g, *g_ln1b, *g_w1, *g_b1, *g_w2, *g_b2, *g_ln2g, *g_ln2b, *g_wl, *g_bl, *g_wl2, *g_bl2;
  void* scratch; size_t scratch_bytes;
  int M, d, dh, dhead, n_vid, nfrm, nppf, nsrl;
  /* round 3, second slice: the same tail for a layer that is NOT followed by the score head (obj_tx, inner mul_tx
   * layers): no_head = 1, d_y [M, d] = gradient of the layer's output (wl / bl / wl2 / d_mdl_outs / dhead unused).
   * y_out (optional, any mode) receives the layer's fp32 output; no_head with d_y == NULL recomputes the forward
   * only (y_out required, no gradient is written). */
  int no_head; const float* d_y; float* y_out;
  /* train-mode dropout of the two sub-layer outputs (ResidualBlock: x + dropout(layer(x)), transformer_code.py:31):
   * probability drop_p (0 = off), masks from the counter-based generator of csrc/train_dev.h (seed, sites drop_site + 1
   * and drop_site + 2, element = row * d + column); forward recomputation and backward use the same masks. */
  float drop_p; unsigned long long drop_seed; int drop_site;
} vog_tail_bwd_args;
/* scratch: caller-owned device memory (4-byte aligned) of at least vog_mul_tail_bwd_scratch_bytes(M, d, dh, no_head ? 0 : dhead)
 * bytes; an entry returns -2 before any launch when scratch_bytes is less. The same contract holds for vog_attn_f32,
 * vog_linear_f32, vog_lang_f32 and vog_score_head_f32_bwd with their own *_scratch_bytes (-1 for a dimension out of range).
 * The sizes are exact: the entry's layout ends at the last byte, nothing behind it is declared or touched. */
int64_t vog_mul_tail_bwd_scratch_bytes(int M, int d, int dh, int dhead);
int vog_mul_tail_bwd(const vog_tail_bwd_args* a, void* stream);

/* Attention + Q / K / V projections of one (Rel)EncoderLayer in fp32 (code/transformer_code.py:136-162, 21-31;
 * box bias code/mdl_vog.py:446-451, 456-490): the other half of the layer's backward (vog_mul_tail_bwd is the
 * tail). x [S*N, d] = layer input, rows (sequence s, token i); token i = arg*n + p, the bias of (p, q) tiled over
 * the N/n argument blocks; heads = torch.chunk(d, n_heads) (unequal and odd sizes allowed); scale sqrt(d).
 *   forward  (d_cat == NULL): cat_out [S*N, d] = concatenated heads softmax((Q K^T + bias) / scale) V.
 *   backward (d_cat != NULL): g_wq / g_wk / g_wv [d, d], g_pe_w [H, 5], g_pe_b [H] (written), d_x [S*N, d] =
 *   (accumulate_dx ? d_x : 0) + dQ Wq + dK Wk + dV Wv; cat_out optional. Any g_* (g_pe_w and g_pe_b together) and d_x
 *   may be NULL: what only they need is skipped.
 * props [S*n, prop_stride >= 5] = (x1, y1, x2, y2, frame) per proposal, normalised by (vid_w, vid_h, vid_w, vid_h,
 * nfrm_div) as compute_pe does; props == NULL: no bias (use_rel off). Activations are recomputed (Q, K, V, the
 * probabilities of one head at a time) in `scratch`. */
typedef struct vog_attn_f32_args {
  const float* x; const float* d_cat;
  const float *wq, *wk, *wv;
  const float* props; int prop_stride; float vid_w, vid_h, nfrm_div;
  const float *pe_w, *pe_b;
  float* cat_out;
  float *g_wq, *g_wk, *g_wv, *g_pe_w, *g_pe_b;
  float* d_x; int accumulate_dx;
  void* scratch; size_t scratch_bytes;
  int S, N, n, d, n_heads;
  /* train-mode dropout on the attention probabilities (transformer_code.py:50, 153): element ((s*H + h)*N + i)*N + j of
   * site drop_site; 0 = off */
  float drop_p; unsigned long long drop_seed; int drop_site;
} vog_attn_f32_args;
int64_t vog_attn_f32_scratch_bytes(int S, int N, int n, int d);
int vog_attn_f32(const vog_attn_f32_args* a, void* stream);

/* The same operator fused (csrc/train_attn.hip): vog_attn_f32's inputs, outputs and dropout masks, but the [S, N, N]
 * probabilities are never stored - one forward launch (online softmax, logits in MFMA accumulators) and two backward launches
 * (dQ + bias partials per query tile; dK, dV per key tile; no atomics, fixed summation order) cover all heads. The Q / K / V
 * projections, the weight-gradient and d_x products stay the GEMMs of vog_attn_f32. Products run on the fp32 MFMA (exact
 * products) or, under the thread's "amp" switch, on the 16-bit MFMA with every operand (Q, K, V, dO, P, dS) rounded to the
 * 16-bit type and everything else fp32; "f32_products" also counts the fused fp32 launches. Head size (d / n_heads rounded
 * up) at most 256.
 *   lse [S, n_heads, N]: the row-wise log-sum-exp of the scaled logits; the forward writes it when it is not NULL.
 *   kept_forward (backward only): lse and cat hold the forward of this very input (same x, weights, boxes, dropout):
 *   the backward starts from them (cat_out must be NULL). Without it the backward first recomputes the forward into
 *   scratch (or into cat_out / lse when given) - both forms give the same bits.
 * scratch: vog_attn_fused_scratch_bytes(S, N, n, d, n_heads) bytes, the contract of the other training entries (exact size,
 * -1 for a dimension out of range, -2 before any launch when scratch_bytes is less): q, k, v, dq, dk, dv, a cat [S*N, d]
 * each, the normalised boxes, delta and lse [S, H, N], 8 floats of bias-gradient partials per (head, sequence, 64-row query
 * tile) - nothing proportional to N^2. */
typedef struct vog_attn_fused_args {
  const float* x; const float* d_cat;
  const float *wq, *wk, *wv;
  const float* props; int prop_stride; float vid_w, vid_h, nfrm_div;
  const float *pe_w, *pe_b;
  float* cat_out;
  float *g_wq, *g_wk, *g_wv, *g_pe_w, *g_pe_b;
  float* d_x; int accumulate_dx;
  void* scratch; size_t scratch_bytes;
  int S, N, n, d, n_heads;
  float drop_p; unsigned long long drop_seed; int drop_site;
  float* lse; const float* cat; int kept_forward;
} vog_attn_fused_args;
int64_t vog_attn_fused_scratch_bytes(int S, int N, int n, int d, int n_heads);
int vog_attn_fused_f32(const vog_attn_fused_args* a, void* stream);

/* Both operators on the FACTORS of mul_tx's layer-0 input instead of the token matrix. Its rows are
 * x[(s, arg, p)] = [ps[(s, p)] | mask * lang[(g(s), arg)]] (vog_conc_f32_fwd) and wq / wk / wv have no bias, so
 *   T[(s, arg, p)] = ps[(s, p)] W_t[:, :dobj]^T + (mask * lang)[(g(s), arg)] W_t[:, dobj:]^T            t in q, k, v:
 * two products over the S*n distinct visual rows and the G*nsrl argument rows, and one launch (vl_expand_kernel) that adds them
 * into the operator's q, k, v. Everything behind that - softmax / fused forward, box bias, dropout, dQ / dK / dV - is the dense
 * entry's. The backward reads dq, dk, dv once (vl_reduce_kernel): dPv_t[(s, p)] = sum_arg dT (ascending arg) and the per-sequence
 * sums over p, which a second launch (vl_reduce_groups_kernel) adds over the sequences of a group in ascending s into
 * dPl_t[(g, arg)] (zero where the mask is 0). No atomics, one fixed order. Then g_w_t[:, :dobj] = dPv_t^T ps, g_w_t[:, dobj:] =
 * dPl_t^T lang, d_ps (+)= sum_t dPv_t W_t[:, :dobj], d_lang (+)= sum_t dPl_t W_t[:, dobj:]. All products are train_gemm.hip's on
 * column blocks of the weights: the thread's amp / bf16_gemm / gemm_amp_pipe switches apply as to the dense products.
 *   ps [S*n, dobj], lang [G*nsrl, dlang], inds_msk [G*nsrl] (int64, NULL = all ones); n_q .. lang_per_vid as vog_conc_f32_fwd /
 *   _bwd take them, with n (the operator's) = nppf: S = n_q*nc_v*nfrm, N = nsrl*n, d = dobj + dlang, G = n_q * (lang_per_vid ?
 *   nc_v : 1), g(s) = s / nfrm (lang_per_vid) | s / (nfrm*nc_v).
 *   d_ps [S*n, dobj], d_lang [G*nsrl, dlang] (backward, each optional: NULL skips its products); accumulate: add to them.
 * With the descriptor the operator's x is not read and its d_x must be NULL; S, N, n, d must agree with it; dlang == 0 is an
 * argument error. scratch: vog_attn_vl_scratch_bytes(...) bytes BESIDE the operator's own scratch, same contract (exact size, -1
 * for a dimension out of range, -2 before any launch when scratch_bytes is less). */
typedef struct vog_attn_vl {
  const float* ps; const float* lang; const int64_t* inds_msk;
  int n_q, nc_v, nfrm, nsrl, dobj, dlang, lang_per_vid;
  float* d_ps; float* d_lang; int accumulate;
  void* scratch; size_t scratch_bytes;
} vog_attn_vl;
int64_t vog_attn_vl_scratch_bytes(int n_q, int nc_v, int nfrm, int n, int nsrl, int dobj, int dlang, int lang_per_vid);
int vog_attn_f32_vl(const vog_attn_f32_args* a, const vog_attn_vl* vl, void* stream);
int vog_attn_fused_f32_vl(const vog_attn_fused_args* a, const vog_attn_vl* vl, void* stream);

/* Backward of concate_vis_lang_feats + the (frame, argument) regroup in front of mul_tx (code/mdl_vog.py:316-344,
 * 681-744). d_x [(q, v, f), (arg, p), dobj + dlang] = gradient of mul_tx's input ->
 *   d_ps   [(q, v), f*nppf + p, dobj]            summed over the arguments,
 *   d_lang [(q, v | 1), arg, dlang] (optional)   summed over the proposals (and the videos when the argument vectors
 *   are shared by them: lang_per_vid == 0), zero where inds_msk [(q, v | 1), arg] (int64, optional) is 0
 *   (retrieve_srl_arg_from_lang_encode's mask, code/mdl_vog.py:138-140). Fixed summation order. */
int vog_conc_f32_bwd(const float* d_x, float* d_ps, float* d_lang, const int64_t* inds_msk, int n_q, int nc_v, int nfrm,
                     int nppf, int nsrl, int dobj, int dlang, int lang_per_vid, void* stream);

/* Linear (+ ReLU) in fp32, forward recomputation and backward: y = act(x W^T + b), x [M, K] (row stride ldx, 0 = K),
 * W [N, K]. dy == NULL: forward only (y required). Otherwise dy [M*rep, ldy] is the gradient of the output rows, each
 * output row having been replicated `rep` times downstream (segment rows over the proposals of their frame,
 * concat_prop_seg_feats code/mdl_conc_single.py:51-66; rep = 1 otherwise; ldy = 0 means N; dy may point into a wider
 * matrix): g_w [N, K], g_b [N], d_x [M, ldx] (accumulate_dx adds); each optional, NULL skips its GEMM. The prop / segment encoders
 * (code/mdl_vog.py:291-314), lstm_out_feat_proj and srl_arg_words_out_enc (:250-283, 97-140). */
typedef struct vog_linear_f32_args {
  const float* x; int64_t ldx; const float *w, *b; int relu;
  float* y;
  const float* dy; int64_t ldy; int rep;
  float *g_w, *g_b, *d_x; int accumulate_dx;
  void* scratch; size_t scratch_bytes;
  int M, N, K;
} vog_linear_f32_args;
int64_t vog_linear_f32_scratch_bytes(int M, int N);
int vog_linear_f32(const vog_linear_f32_args* a, void* stream);

/* Language side in fp32, forward recomputation and backward: token re-index (get_srl_arg_seq_to_sent_seq
 * code/mdl_vog.py:67-95) -> embedding -> packed multi-layer BiLSTM (LSTMEncoder utils/mdl_srl_utils.py:114-169) ->
 * lstm_out_feat_proj on every step (code/mdl_vog.py:250-283) -> argument vectors relu(W [h(start) | h(end)] + b)
 * (retrieve_srl_arg_from_lang_encode :97-140, before the argument mask).
 *   words_ind [Bn, words_len], word_mask [Bn, mask_len], lens [Bn], capture [Bn, nsrl, 2]: int64, device, as vog_batch;
 *   T = longest sentence of the batch; emb [vocab_size + 1, E]; w_ih[l][dir] [4R, E | 2R], w_hh [4R, R], b_* [4R]
 *   (dir 0 = forward, 1 = reverse; gate order i, f, g, o); w_proj [D, 2R]; w_arg [L, 2D].
 *   d_lang_enc == NULL: forward only (lang_enc_out [Bn*nsrl, L] and / or full_out [Bn*T, D]).
 *   Otherwise d_lang_enc [Bn*nsrl, L] = gradient of the argument vectors (already masked) and every non-NULL g_* is
 *   written: back-propagation through time with packed-sequence semantics (a sentence's state is frozen past its length,
 *   its outputs there are zero). A NULL g_* is a frozen weight: its GEMM is skipped, and so is the part of the chain
 *   that reaches no wanted gradient (the layers below the lowest one with a non-NULL g_*, when g_emb is NULL too).
 *   d_hid (optional, [Bn, D], with d_lang_enc) = gradient of hid_out, the projection of final_hidden that feeds the sep
 *   verb head: its backward adds to g_w_proj / g_b_proj, and d final_hidden enters the top layer's back-propagation as
 *   the gradient of the forward direction's state after step len-1 and of the reverse direction's after position 0. */
typedef struct vog_lang_f32_args {
  const int64_t *words_ind, *word_mask, *lens, *capture;
  int Bn, nsrl, words_len, mask_len, T, vocab_size, E, R, layers, D, L;
  const float* emb;
  const float* w_ih[4][2]; const float* w_hh[4][2]; const float* b_ih[4][2]; const float* b_hh[4][2];
  const float *w_proj, *b_proj, *w_arg, *b_arg;
  const float* d_lang_enc;
  float *lang_enc_out, *full_out;
  float* g_emb;
  float* g_w_ih[4][2]; float* g_w_hh[4][2]; float* g_b_ih[4][2]; float* g_b_hh[4][2];
  float *g_w_proj, *g_b_proj, *g_w_arg, *g_b_arg;
  void* scratch; size_t scratch_bytes;
  float* hid_out;   /* optional [Bn, D]: lstm_out_feat_proj(final_hidden[-1]) - the verb feature of the sep head */
  /* train-mode dropout of LSTMEncoder (utils/mdl_srl_utils.py:104, 128, 150): drop_in on the embedded tokens (site 1),
   * drop_out behind every BiLSTM layer (site 2 + l between layers, 10 on the output); 0 = off */
  float drop_in, drop_out; unsigned long long drop_seed;
  /* 1: `scratch` still holds the forward of an earlier call with the same inputs, weights and dropout seed (no other call used
   * the buffer in between): the backward starts from those activations instead of recomputing them */
  int reuse_forward;
  const float* d_hid;
} vog_lang_f32_args;
/* (the size follows the calling thread's "amp" and "lstm_fused" switches, vog_train_set_int) */
int64_t vog_lang_f32_scratch_bytes(int Bn, int T, int nsrl, int E, int R, int layers, int D, int L);
int vog_lang_f32(const vog_lang_f32_args* a, void* stream);

/* The remaining forward pieces of the fp32 training path (the forward vog_*_bwd differentiate, kept in fp32 with
 * its activations; the 16-bit inference forward above keeps none):
 *   vog_concat_rows_f32: out[m, :Na] = a[m / rep_a], out[m, Na:] = b[m / rep_b] (concat_prop_seg_feats: rep_b = nppf0);
 *   vog_conc_f32_fwd:    mul_tx's input from obj_tx's output and the (masked) argument vectors - the forward of
 *                        vog_conc_f32_bwd, same argument meaning;
 *   vog_score_head_f32:  mdl_outs [n_vid, nsrl, nfrm*nppf] = lin2(y) regrouped (code/mdl_vog.py:224-230, 724-737),
 *                        scratch >= M * dhead * 4 bytes.
 * vog_adam_f32: one torch.optim.Adam step (no weight decay / amsgrad - those are vog_opt_step_ex_f32's; the reference uses betas (0.9, 0.99),
 * code/main_dist.py:55) on one parameter tensor; step counts from 1. */
int vog_concat_rows_f32(const float* a, int Na, int rep_a, const float* b, int Nb, int rep_b, float* out, int M, void* stream);
int vog_conc_f32_fwd(const float* ps, const float* lang, const int64_t* inds_msk, float* out, int n_q, int nc_v, int nfrm, int nppf,
                     int nsrl, int dobj, int dlang, int lang_per_vid, void* stream);
int vog_score_head_f32(const float* y, const float* wl, const float* bl, const float* wl2, const float* bl2, float* mdl_outs,
                       void* scratch, size_t scratch_bytes, int M, int d, int dhead, int n_vid, int nfrm, int nppf, int nsrl,
                       void* stream);
int vog_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int step,
                 void* stream);
/* The optimiser step of a whole parameter set in a few launches (csrc/optim.hip): torch.optim.Adam as vog_adam_f32 computes it,
 * optionally behind the gradient statistics that loss scaling (torch.amp.GradScaler) and gradient clipping
 * (torch.nn.utils.clip_grad_norm_) need. `tensors` is a HOST array of n_tensors quadruples of device pointers (fp32, 4-byte
 * aligned, n elements each; 16-byte accesses wherever the four share their alignment, one element per lane otherwise); the
 * launches carry it in their kernel arguments, so it may change from call to call (the gradient pointers do).
 *   Mode A (state == NULL): plain Adam with the host-counted `step` (>= 1). Bit-identical to vog_adam_f32 per tensor.
 *   Mode B (state != NULL): three stages on the stream, nothing read back by the host.
 *     1. statistics: sum over all tensors of (g / scale)^2 - one partial per workgroup, fixed-order sums, no atomics (the same
 *        bits on every run and every rank);
 *     2. finalise: the partials are added in double; grad_norm = sqrt(sum); found_inf = the sum is not finite;
 *        clip = max_norm > 0 ? min(1, max_norm / (grad_norm + 1e-6)) : 1; coef = clip / scale; then GradScaler.update:
 *        on overflow scale *= backoff_factor, growth_tracker = 0, skipped += 1, adam_step stays; otherwise adam_step += 1,
 *        growth_tracker += 1 and, when it reaches growth_interval, scale *= growth_factor and the tracker returns to 0
 *        (growth_interval <= 0: the scale never changes; an overflowing step is still skipped). The bias corrections of the
 *        new adam_step are computed here, once;
 *     3. apply: nothing is written when found_inf is set (p, m, v keep their bits); otherwise Adam on g * coef.
 *   `state` is 32 bytes of device memory that the caller owns and initialises (scale > 0; counters as they should continue);
 *   `scratch` (mode B only) is device memory of at least vog_opt_scratch_bytes(n_tensors, sum of n) bytes, 8-byte aligned.
 *   A gradient whose unscaled square leaves the fp32 range counts as overflow.
 * vog_opt_scale_grad_f32: x[i] *= state->scale on the device (the seed gradient of a scaled backward).
 * vog_opt_step_groups_f32: the same step with PARAMETER GROUPS (torch.optim's param_groups): group k covers tensors
 *   [first, first + count) of base.tensors with its own lr and weight_decay. Groups are disjoint, ascending and non-empty
 *   (anything else is an argument error before any launch). A tensor no group covers is FROZEN: it is in no launch, its
 *   p / g / m / v are neither read nor written (nor validated), and it takes no part in mode B's statistics - grad_norm,
 *   clipping and the overflow decision cover the grouped tensors only. base.lr is ignored; beta1 / beta2 / eps, the loss-scale
 *   fields and `state` are shared by all groups. weight_decay is torch.optim.Adam's L2 form here (AdamW's decoupled decay is
 *   VOG_OPT_DECOUPLED of vog_opt_step_ex_f32, below):
 *   the gradient that enters the moments is fma(weight_decay, p, g * coef), coef = mode B's clip / scale (1 in mode A) - one
 *   fused multiply-add; the decay is not part of the statistics (clip_grad_norm_ runs before optimizer.step). The launch
 *   tables are cut at group boundaries; given `coef`, a tensor's bits do not depend on which launch carries it (mode A: never;
 *   mode B: grad_norm is a fixed-order sum over the launches' partials, so its last bits, and with them coef, depend on the
 *   grouping - not on the run or the rank). Scratch of
 *   vog_opt_scratch_bytes(base.n_tensors, sum of every n) bytes is sufficient for any grouping. vog_opt_step_f32 is one group
 *   over every tensor with base.lr and no decay, on the same code path.
 * vog_opt_step_ex_f32: the grouped step (`groups`: everything above holds - modes A and B, frozen tensors, tables cut at group
 *   boundaries) with torch 2.10's _single_tensor_adam variants, per call:
 *     flags       VOG_OPT_DECOUPLED: a group's weight_decay is AdamW's - p *= 1 - lr * weight_decay (the factor formed in double,
 *                   rounded once) in front of the moments, the gradient is left alone;
 *                 VOG_OPT_AMSGRAD: vmax = max(vmax, v) is stored and the denominator is sqrt(vmax) / sqrt(bc2) + eps;
 *                 VOG_OPT_MAXIMIZE: the gradient is negated. Any other bit is an argument error.
 *     vmax        HOST array of n_tensors device pointers, parallel to `tensors` (fp32, 4-byte aligned, n elements): read,
 *                 required and validated only with VOG_OPT_AMSGRAD, and only for grouped tensors (a NULL or misaligned entry
 *                 there is an argument error before any launch). 16-byte accesses need all FIVE pointers to agree.
 *     grad_scale  > 0, finite: the gradient is multiplied by it - 1 / (micro-batches of an accumulation window) turns summed
 *                 gradients into their mean. It forms ONE factor with mode B's coef (and MAXIMIZE's sign): g * (coef * grad_scale).
 *   Order per element: g * factor; L2 decay g = fma(wd, p, g) or decoupled p *= 1 - lr * wd; m, v with vog_adam_f32's roundings;
 *   vmax; p. Mode B's statistics see g * grad_scale / scale - the averaged gradient, which is what clip_grad_norm_ would see -
 *   before decay and whatever the sign; an overflowing step writes nothing, vmax included. With flags == 0 and grad_scale == 1
 *   the call IS vog_opt_step_groups_f32 (the same launches, the same bits). With vmax a launch carries 16 tensors, not 20; given
 *   coef, a tensor's bits do not depend on which launch carries it.
 * vog_opt_accum_f32: acc[i] += g[i] over a HOST table of n_tensors (acc, g, n) triples of device pointers (fp32, 4-byte aligned;
 *   any number of tensors, 32 per launch) - the sum of a gradient-accumulation window. 16-byte accesses where acc and g share
 *   their alignment, one element per lane otherwise; every element is added once by one lane: no atomics, one rounding. */
typedef struct vog_opt_tensor { float* p; const float* g; float* m; float* v; int64_t n; } vog_opt_tensor;
typedef struct vog_opt_state {
  float scale;            /* loss scale the gradients carry (1 = none) */
  int growth_tracker;     /* clean steps since the last change of scale */
  int adam_step;          /* steps APPLIED so far (bias correction) */
  int found_inf;          /* last call: 1 = a gradient was non-finite, the step was skipped */
  float grad_norm;        /* last call: L2 norm of all unscaled gradients, before clipping */
  float coef;             /* last call: factor applied to every gradient = clip / scale (0 on a skipped step) */
  int skipped;            /* steps skipped so far */
  int reserved;
} vog_opt_state;
typedef struct vog_opt_args {
  const vog_opt_tensor* tensors; int n_tensors;
  float lr, beta1, beta2, eps;
  int step;                   /* mode A only */
  vog_opt_state* state;       /* NULL = mode A */
  float max_norm;             /* <= 0: no clipping */
  float growth_factor, backoff_factor; int growth_interval;
  void* scratch; size_t scratch_bytes;
} vog_opt_args;
int64_t vog_opt_scratch_bytes(int n_tensors, int64_t total_elems);
int vog_opt_step_f32(const vog_opt_args* a, void* stream);
typedef struct vog_opt_group { int first, count; float lr, weight_decay; } vog_opt_group;   /* tensors [first, first + count) of the table */
typedef struct vog_opt_groups_args { vog_opt_args base; const vog_opt_group* groups; int n_groups; } vog_opt_groups_args;
int vog_opt_step_groups_f32(const vog_opt_groups_args* a, void* stream);
int vog_opt_scale_grad_f32(float* x, int64_t n, const vog_opt_state* state, void* stream);
#define VOG_OPT_DECOUPLED 1u
#define VOG_OPT_AMSGRAD 2u
#define VOG_OPT_MAXIMIZE 4u
typedef struct vog_opt_ex_args { vog_opt_groups_args groups; unsigned flags; float* const* vmax; float grad_scale; } vog_opt_ex_args;
int vog_opt_step_ex_f32(const vog_opt_ex_args* a, void* stream);
typedef struct vog_opt_accum_tensor { float* acc; const float* g; int64_t n; } vog_opt_accum_tensor;
int vog_opt_accum_f32(const vog_opt_accum_tensor* tensors, int n_tensors, void* stream);
/* vog_opt_average_f32: WEIGHT AVERAGING behind the optimiser step, on the same stream - torch.optim.swa_utils.AveragedModel with
 * get_ema_multi_avg_fn(decay) (VOG_AVG_EMA) or get_swa_multi_avg_fn() (VOG_AVG_SWA): avg = lerp(avg, p, w), the first update a copy.
 * Whether this call averages at all is decided on the device (one workgroup, lane 0) and nothing is read back by the host:
 *     s = opt_state ? opt_state->adam_step : step          (mode B: the optimiser's block, as the step just left it | mode A)
 *     skip when (opt_state && opt_state->found_inf) or s < start or (s - start) % every != 0:
 *         w = 0, updated = 0, n_averaged stays, no average is read or written;
 *     otherwise, with n = n_averaged:  w = 1 (n == 0) | 1 / (n + 1) (SWA) | 1 - decay_eff (EMA), formed in double and rounded to
 *         float once, decay_eff = warmup ? min(decay, (1 + n) / (10 + n)) : decay;  then n_averaged = n + 1, updated = 1.
 *   So a step that mode B skipped does not average, and the schedule follows the count of APPLIED steps, not of calls.
 *   Apply: w == 1 stores p's bits; otherwise avg = fmaf(w, p - avg, avg) (two roundings per update; earlier errors never grow,
 *   0 <= 1 - w <= 1). `tensors` is a HOST table of (avg, p, n) triples of device pointers (fp32, 4-byte aligned, any number,
 *   32 per launch): 16-byte accesses where avg and p share their alignment, one element per lane otherwise; every element is
 *   written by one lane - no atomics, the same bits on every run and every rank. p is never written.
 *   `state` is 16 bytes of device memory that the caller owns and initialises (zeros for a fresh average). Argument errors (before
 *   any launch): a NULL / misaligned pointer, n <= 0, an unknown mode, EMA's decay outside [0, 1] or not finite, start < 1,
 *   every < 1, mode A with step < 1, a NULL state.
 *   The pass is separate from the optimiser's apply kernels on purpose: their instructions, and with them the bits of a step
 *   without averaging, stay what they were (fusing would save one read of p, a third of this pass's traffic). */
#define VOG_AVG_EMA 1
#define VOG_AVG_SWA 2
typedef struct vog_opt_avg_tensor { float* avg; const float* p; int64_t n; } vog_opt_avg_tensor;
typedef struct vog_opt_avg_state {   /* 16 bytes of device memory, owned and initialised by the caller */
  int n_averaged;                    /* averaging updates applied so far */
  int updated;                       /* last call: 1 = the averages moved */
  float w;                           /* last call: the interpolation weight used (0 = none) */
  int reserved;
} vog_opt_avg_state;
typedef struct vog_opt_avg_args {
  const vog_opt_avg_tensor* tensors; int n_tensors;   /* HOST table of device pointers, fp32, 4-byte aligned */
  int mode;                          /* VOG_AVG_EMA | VOG_AVG_SWA */
  double decay;                      /* EMA only, in [0, 1] */
  int warmup;                        /* EMA only: decay_eff = min(decay, (1 + n) / (10 + n)), n = n_averaged before the update */
  int start, every;                  /* average on applied step s when s >= start and (s - start) % every == 0; start >= 1, every >= 1 */
  const vog_opt_state* opt_state;    /* mode B: the optimiser's device block; NULL = mode A */
  int step;                          /* mode A: the applied-step count of the step just made (>= 1) */
  vog_opt_avg_state* state;
} vog_opt_avg_args;
int vog_opt_average_f32(const vog_opt_avg_args* a, void* stream);
/* Backward of vog_score_head_f32 alone (ImgGrnd / VidGrnd: lin2 reads the [vis | lang] token matrix directly,
 * code/mdl_vog.py:224-230, 286-344): g_wl [dhead, d], g_bl [dhead], g_wl2 [dhead], g_bl2 [1], d_x [M, d] (each optional). */
int64_t vog_score_head_f32_bwd_scratch_bytes(int M, int d, int dhead);
int vog_score_head_f32_bwd(const float* x, const float* d_mdl_outs, const float* wl, const float* bl, const float* wl2,
                           float* g_wl, float* g_bl, float* g_wl2, float* g_bl2, float* d_x, void* scratch, size_t scratch_bytes,
                           int M, int d, int dhead, int n_vid, int nfrm, int nppf, int nsrl, void* stream);
/* Switches of the training path. "bf16_gemm" = 1: the tile GEMMs of vog_*_f32 / vog_*_bwd round their operands to bf16 and
 * use the 16-bit matrix instruction with fp32 accumulation (mixed precision: faster, gradients within ~1e-2 of the fp32
 * ones); 0 (default): fp32 operands, the path pinned against autograd through the reference.
 * The switch belongs to the CALLING THREAD (thread-local; no process-wide state): it selects the kernels of the vog_*_f32 /
 * vog_*_bwd calls that thread issues afterwards. A trainer sets it at the top of every step (train.FP32Trainer), so two
 * trainers with different settings - in one thread or in two - never see each other's choice.
 * "amp" = 1 (bf16) | 2 (f16) | 0 (off, default): mixed precision as torch.autocast does it - EVERY product the training path
 * issues (tile, split-K and weight-stream forms, any operand layout, and the BiLSTM recurrence of vog_lang_f32, which then runs
 * fused: one launch per layer and step for both directions, from 16-bit copies of W_hh / W_hh^T made once per call) takes 16-bit
 * operands with fp32 accumulation; softmax, LayerNorm, the cell nonlinearities, dropout, column sums, the loss and Adam stay
 * fp32. Other values are refused. Same thread-local contract as bf16_gemm, which it overrides. vog_lang_f32_scratch_bytes
 * follows the calling thread's "amp" (the two 16-bit weight copies: 16 R^2 bytes per layer and direction, 64 MB at R = 1024
 * with 2 layers), so query it with the switch set as it will be for the call.
 * "f32_products": the number of fp32 product kernels the calling thread has launched, the fp32 instantiations of
 * vog_attn_fused_f32's kernels included (read-only counter; writing 0 resets it).
 * "lstm_fused" = 1 | 0 (default): the fp32 BiLSTM recurrence of vog_lang_f32, forward and backward, in ONE launch per layer and
 * step for both directions (the recurrent product in exact fp32 on the matrix pipe, K split over the waves of a workgroup and
 * summed in a fixed order, then the cell) instead of a product and a cell launch per direction and step. Same thread-local
 * contract; other values are refused. With "amp" != 0 it changes nothing (amp has fused kernels of its own); "bf16_gemm" keeps
 * fp32 recurrent products and so takes these kernels. vog_lang_f32_scratch_bytes follows it as it follows "amp" (the second
 * direction's dG by step and by position, its dc and its W_hh^T: 8 Bn T R + Bn R + 4 R^2 floats), and a backward with
 * reuse_forward starts from a forward made with the same setting.
 * "lstm_fused_launches": the number of launches of those two kernels by the calling thread (read-only counter; writing 0
 * resets it).
 * "lstm_amp_split" = 1 | 0 (default): under "amp" != 0, the BiLSTM recurrence of vog_lang_f32 in kernels that split K over the
 * waves of a workgroup (forward: 4 units x 4 gates x 16 sentences per workgroup, K = R over 4 waves; backward: 16 units x 16
 * sentences, K = 4R over 16 waves; the partial sums added in wave order) instead of the tile kernels (16 units per workgroup, a
 * wave a whole gate and all of K). Every operand is rounded where the tile kernels round it (h and dG per fragment from fp32,
 * W_hh from the same 16-bit copies) and accumulation is fp32: only the order of the fp32 sums differs. Same thread-local
 * contract; other values are refused. With "amp" == 0 it changes nothing (bits, launches, the counter stays 0), and
 * "lstm_fused" keeps its contract under amp. Buffers and scratch layout are the tile kernels': vog_lang_f32_scratch_bytes does
 * not depend on it, and a backward with reuse_forward may start from a forward made with either setting.
 * "lstm_amp_split_launches": the number of launches of those two kernels by the calling thread (read-only counter; writing 0
 * resets it).
 * "gemm_amp_pipe" = 1 | 0 (default): under "amp" != 0, every product that takes the vector 128 x 64 tile kernel (all four operand
 * layouts, batches, split-K partials, bias / relu / accumulate) runs in the pipelined tile kernel instead: 64-wide K episodes in
 * two LDS buffers with one barrier each, the next episode's operands in registers meanwhile, on 64 x 64 tiles. Operands, rounding, matrix instruction, order of the 32-wide K chunks and epilogue are
 * the tile kernel's, so the results are the same bits. The split-K decision, the element-wise tile (odd dimensions, strides or
 * alignments), the weight-stream kernel and "bf16_gemm" are as they were. Same thread-local contract; other values are refused.
 * With "amp" == 0 it changes nothing (bits, launches, the counter stays 0), and no *_scratch_bytes function depends on it.
 * "gemm_amp_pipe_launches": the number of launches of that kernel by the calling thread (read-only counter; writing 0 resets
 * it).
 * "attn_fused_pipe" = 1 | 0 (default): vog_attn_fused_f32 issues the pipelined forms of its forward, dQ and dK / dV kernels
 * (fp32, bf16 and f16; every head size): staged tiles of several arithmetic sub-tiles in two LDS buffers with one barrier
 * each, the next tile's rows in registers meanwhile, 16-byte staging where the head's column offset allows it, no workgroup
 * barrier around the wave-private probability tiles, transposed LDS reads of the 16-bit strided operand. Sub-tile, matrix
 * instruction, assignment of k to lane and element, rounding points and every summation order are those of the plain
 * kernels, so cat, lse, delta and every gradient are the same bits. Arguments, projections, weight-gradient products, the
 * bias-gradient sum and vog_attn_fused_scratch_bytes do not depend on it. Same thread-local contract; other values are
 * refused. No effect on any other entry.
 * "attn_fused_pipe_launches": the number of launches of those three kernels by the calling thread (read-only counter;
 * writing 0 resets it).
 * "attn_vl_launches": the number of launches of vl_expand_kernel, vl_reduce_kernel and vl_reduce_groups_kernel (the kernels
 * vog_attn_f32_vl / vog_attn_fused_f32_vl add to the dense operators) by the calling thread (read-only counter; writing 0 resets
 * it). */
int vog_train_set_int(const char* name, int value);
int vog_train_get_int(const char* name, int* value);
/* ---- the CAPTURED training step (train.FP32Trainer.capture): one graph launch per iteration. A replayed launch cannot take a
 * per-step value from its kernel arguments, so everything that changes from step to step lives in device memory.
 *
 * vog_train_step: 16 bytes of device memory, 8-byte aligned, owned and initialised by the caller.
 *   tick        the iteration count at the START of the step (the trainer's num_it): numbers the dropout masks;
 *   adam_step   the count of APPLIED plain-Adam updates (mode A of vog_opt_step_dev_f32; mode B counts in vog_opt_state);
 *   len_clamped sticky: set to 1 by VOG_TICK_BEGIN when a sentence length exceeded T, never cleared by the library.
 * vog_train_tick, one launch of one workgroup, every word written by a plain vector store (no atomics):
 *   phase VOG_TICK_BEGIN - the first node of a step: lens[i] = min(lens[i], T) IN PLACE over the n_lens int64 lengths of the
 *     step's static input buffer, and len_clamped = 1 if any was larger. The language kernels behind it never see a length
 *     beyond the T their launches were sized for: a clamped step computes a truncated sentence (wrong, but inside its buffers),
 *     and the sticky word reports it. capture (optional, n_capture int64 values: vog_lang_f32's `capture`, the positions the
 *     argument vectors are gathered from) is clamped to [0, T - 1] the same way - those index the T rows of a sentence.
 *     lens == NULL with n_lens == 0 (no language stage in the step): no launch.
 *   phase VOG_TICK_END - the last node, behind the optimiser and the averaging: row tick % log_rows of the ring loss_log
 *     [log_rows][n_loss + 1] takes the n_loss fp32 values at loss_src and, as word n_loss, the marker (uint32)(tick + 1) - this
 *     step's row only (a zero-filled ring has no valid row) -, then tick += 1 and, with count_adam, adam_step += 1. loss_log
 *     NULL: only the counts. Forward and backward of one step read the same tick, because it advances here.
 * vog_train_set_ptr: the calling thread's POINTER switches, beside vog_train_set_int and under the same thread-local contract.
 *   "drop_tick" = a device pointer to a vog_train_step's tick (8-byte aligned) | NULL (default): while it is set, the drop_seed
 *   of vog_attn_f32 / vog_attn_fused_f32 / vog_mul_tail_bwd / vog_lang_f32 is the BASE of the seed and every mask is drawn with
 *   seed = (drop_seed + *tick) & (2^63 - 1), read on the device by the kernels themselves. With base = dropout_seed * 1000003 + 1
 *   (mod 2^64) that is the seed train.FP32Trainer hands over for num_it = tick, bit for bit. The argument structs keep their layout.
 * vog_train_pin_scratch: the split-K partial buffer of `stream` (one per stream, grown on demand by the products of the
 *   training path) is pinned (on != 0) or released. While it is pinned - and on any stream that is being captured - a product
 *   that needs more than the buffer holds fails with -3 and a message and neither allocates nor frees: a captured graph
 *   keeps pointing into the buffer it was captured with. vog_train_scratch_info reports the buffer (each output optional).
 * Launch counters (vog_train_get_int's *_launches) count calls of the library, so under capture they count once, at capture,
 * and not per replay. */
typedef struct vog_train_step { long long tick; int adam_step; int len_clamped; } vog_train_step;
enum { VOG_TICK_BEGIN = 0, VOG_TICK_END = 1 };
int vog_train_tick(vog_train_step* step, int64_t* lens, int n_lens, int T, const float* loss_src, float* loss_log, int log_rows,
                   int n_loss, int phase, int count_adam, int64_t* capture, int n_capture, void* stream);
int vog_train_set_ptr(const char* name, const void* value);
int vog_train_pin_scratch(void* stream, int on);
int vog_train_scratch_info(void* stream, void** ptr, size_t* bytes, int* pinned);
/* "kernel_fills" (vog_train_set_int) = 1 | 0 (default): the device fills and copies inside vog_lang_f32 and vog_mul_tail_bwd are
 * kernels instead of hipMemsetAsync / hipMemcpyAsync / hipMemcpy2DAsync - the same bytes - so that a step recorded with the
 * switch on is a chain of kernel nodes only. Same thread-local contract as the other switches.
 * vog_graph_node_count: *n = the number of nodes of a captured graph (a hipGraph_t). */
int vog_graph_node_count(void* graph, int* n);
/* The optimiser without per-step host scalars (what a captured step replays).
 * vog_opt_step_dev_f32: vog_opt_step_ex_f32 (same argument block, same checks, tables and launches; flags 0 and grad_scale 1 is
 *   the grouped step) whose apply launches read from DEVICE memory what the host entries pass as kernel arguments:
 *   lr        one float per group, in group order (groups[k].lr is not read). The caller rewrites it with a stream-ordered
 *             copy when a schedule moves a rate. AdamW's factor is formed on the device as (float)(1.0 - (double)lr * (double)wd),
 *             the host's expression on an exact double product: the same bits.
 *   step      mode A (base.state == NULL; base.step is not read): the update applied is number step->adam_step + 1; the count
 *             itself is advanced by vog_train_tick(VOG_TICK_END, count_adam = 1) behind the last launch that reads it.
 *   bias      mode A: the (bc1, bc2_sqrt) pairs of vog_opt_bias_table in device memory, bias_len of them; update s reads
 *             entry min(s, bias_len) - 1. With the table complete (its last entry is (1, 1)) p, m, v are the bits of the host
 *             entries for every s.
 *   Mode B decides and counts on the device already: only lr moves to the table; step / bias are not read.
 * vog_opt_bias_table (HOST function, no device call): out[2 (s - 1)] = 1.f - powf(beta1, (float)s), out[2 (s - 1) + 1] =
 *   sqrtf(1.f - powf(beta2, (float)s)) - mode A's own expressions - for s = 1 .. *len, where *len is the first s at which both are
 *   1.0f. Returns -2 (out holds the first cap entries, *len the count needed) when *len > cap, and when it would pass 2^20.
 * vog_opt_average_dev_f32: vog_opt_average_f32 whose mode A takes the count from the step block (step->adam_step + 1, in front
 *   of VOG_TICK_END) instead of a->step. With a->opt_state (mode B) it is vog_opt_average_f32 itself. */
typedef struct vog_opt_dev_args { const float* lr; const vog_train_step* step; const float* bias; int bias_len; } vog_opt_dev_args;
int vog_opt_step_dev_f32(const vog_opt_ex_args* a, const vog_opt_dev_args* d, void* stream);
int vog_opt_bias_table(float beta1, float beta2, float* out, int cap, int* len);
int vog_opt_average_dev_f32(const vog_opt_avg_args* a, const vog_train_step* step, void* stream);
/* out[g, n] = mean over f of x[g, f, n] (the segment mean of the sep verb head, code/mdl_conc_sep.py:64-129) */
int vog_row_mean_f32(const float* x, float* out, int G, int F, int N, void* stream);
/* Backward of the evaluation scores mdl_outs_eval = sigmoid(mdl_outs) * arg_msk * cmp_msk (code/mdl_conc_single.py:118-122,
 * mdl_conc_sep.py:200-210), fused with the gradient that reaches mdl_outs directly:
 *   d_logits = d_outs + d_eval * s (1 - s) * arg_msk * cmp_msk,  s = sigmoid(logits),
 * all [n_vid, nsrl, NP] fp32 (n_vid = B * nc_v); d_outs / d_eval may be NULL (= 0). The masks (int64) are broadcast as
 * vog_score_head does: arg_msk [B, nvl, nsrl] (nvl = 1 or nc_v), cmp_msk [B, ncmp] by the comparison video of each
 * proposal row (temp: frame block, spat: proposal block, sep / svsq: the video). */
int vog_score_eval_bwd_f32(const float* logits, const float* d_outs, const float* d_eval, const int64_t* arg_msk, const int64_t* cmp_msk,
                           float* d_logits, int n_vid, int nsrl, int NP, int conc_type, int ncmp, int nc_v, int nvl, int nfrm0, int nppf0,
                           void* stream);
/* out[m, c] = sum_{j < rep} x[(m*rep + j) * ldx + c] + (y ? y[(m / F) * ldy + c] / F : 0), out [M, N] fp32: the gradient of
 * a row that was replicated `rep` times downstream, plus that of a mean over groups of F rows. The segment encoder's output
 * gradient of the sep verb head (its nppf0 replicas in the [prop | seg] rows and the segment mean, code/mdl_conc_sep.py:64-129)
 * and the gradient of final_hidden shared by the videos of a query. */
int vog_rep_sum_f32(const float* x, int64_t ldx, int rep, const float* y, int64_t ldy, int F, float* out, int M, int N, void* stream);

/* ------------------------------------------------------------------------- *
 * Whole forward (replaces Conc{TEMP,SPAT,SEP}.forward + the evaluator head)
 * ------------------------------------------------------------------------- */
typedef struct vog_model_desc {
  int mdl_kind, conc_type;
  int vocab_size, emb_dim, rnn_size, rnn_layers;
  int prop_dim, seg_dim, prop_enc, seg_enc, lang_enc;
  int obj_layers, obj_heads, obj_use_rel, obj_one_frm, obj_to_use;
  int mul_layers, mul_heads, mul_use_rel;
  int nfrm0, nppf0, nsrl, seq_len;
  float vid_w, vid_h;
  int tx_dtype;      /* vog_dtype of the two transformers */
  int enc_dtype;     /* vog_dtype of LSTM / encoders / score head (default f16) */
} vog_model_desc;

typedef struct vog_ctx vog_ctx;
int vog_ctx_create(const vog_model_desc* d, vog_ctx** out);
int vog_ctx_set_weight(vog_ctx* c, const char* name, const float* host, int64_t numel);
int vog_ctx_finalize(vog_ctx* c);          /* synchronous; uploads + converts */
int vog_ctx_destroy(vog_ctx* c);
int vog_ctx_num_weights(const vog_ctx* c); /* names the model expects */
const char* vog_ctx_weight_name(const vog_ctx* c, int i);
int64_t vog_ctx_weight_numel(const vog_ctx* c, int i);

/* ---- weight images, in-place refresh from device parameters ---------------------------------------------------------
 * vog_ctx_finalize keeps a table with one row per device buffer it makes: where the buffer is, how many bytes, and how it
 * derives from the weights. The rows are read-only; they change only when vog_ctx_finalize runs again. */
typedef enum {
  VOG_IMG_F32 = 0,          /* plain fp32 copy */
  VOG_IMG_CAST16 = 1,       /* plain 16-bit cast */
  VOG_IMG_QKV_PAD = 2,      /* head-padded [3 * H * dp, nk] image of columns [k0, k0 + nk) of Wq / Wk / Wv, row-major */
  VOG_IMG_WO_PAD = 3,       /* head-padded [d, H * dp] Wo, row-major */
  VOG_IMG_FRAG16 = 4,       /* 16x32 fragment order (vog_pack_w_frag) of a weight, of padded QKV columns or of [W_fwd ; W_bwd] */
  VOG_IMG_FRAG32 = 5,       /* 32x16 fragment order (vog_pack_w_frag32) of a weight, of the padded QKV rows or of the padded Wo */
  VOG_IMG_LSTM_PACK = 6,    /* BiLSTM tile order of both directions (vog_lstm_pack_w / _whh) */
  VOG_IMG_WIH_CAT = 7,      /* [W_ih_fwd ; W_ih_bwd], 16 bit, row-major */
  VOG_IMG_BIAS_SUM = 8,     /* b_ih + b_hh of both directions, fp32 */
  VOG_IMG_GATE_TABLE = 9    /* layer 0's gate inputs for the whole vocabulary (vog_lstm_layer_args.gx_table) */
} vog_image_kind;
#define VOG_IMAGE_MAX_SRC 8
typedef struct vog_image_info {
  const char* name;         /* stable: "mult_txf.0.wqkv_p", "lstm.1.wih_f", "gx0_tab", ... (owned by the context) */
  const void* dev;
  int64_t bytes;
  int kind;                 /* vog_image_kind */
  int dtype;                /* vog_dtype, -1: fp32 */
  int lo;                   /* 1: the image holds the 16-bit remainders t16(w - back(t16(w))) of a hi + lo pair */
  int n_src;
  const char* src[VOG_IMAGE_MAX_SRC];   /* the weights it is made from */
} vog_image_info;
int vog_ctx_num_images(const vog_ctx* c);          /* -1 unless finalized */
int vog_ctx_image_info(const vog_ctx* c, int i, vog_image_info* out);

/* Rewrite the images of a FINALIZED context in place from fp32 device tensors, with the pack kernels of csrc/wpack.hip on
 * `stream`: the addresses stay (captured graphs stay valid) and the bytes are the ones vog_ctx_finalize makes from the same
 * finite values (NaN weights are out of scope). Names go through the normalisation of vog_ctx_set_weight. `srcs` may be a
 * subset: an image is rewritten when at least one of its sources is named, and then needs all of them (bias sums,
 * [W_ih_fwd ; W_ih_bwd], the gate table). Everything is validated before the first launch: an unknown name, a wrong numel, a
 * NULL pointer or a context that is not finalized returns < 0 with vog_last_error set and nothing written. The call does
 * not wait for the device and, after the first call on a context, does not allocate; the caller orders it against forwards
 * in flight. The host copies of the refreshed weights become stale: vog_ctx_finalize fails, naming the first of them, until
 * vog_ctx_set_weight has supplied them again. */
typedef struct vog_weight_src { const char* name; const float* dev; int64_t numel; } vog_weight_src;
int vog_ctx_refresh_device(vog_ctx* c, const vog_weight_src* srcs, int n, void* stream);

/* Host only: out[i] = row-major source index of the element a packer puts at destination position i - the shared placement
 * rules (csrc/wpack_dev.h) that the host packers and the device pack kernels both call. layout 1: vog_pack_w_frag of [N, K];
 * 2: vog_pack_w_frag32 of [N, K]; 3: vog_lstm_pack_w with R = N, source [W_fwd ; W_bwd] = [8 * R, K] (8 * R * K entries). */
int vog_wpack_index_map(int layout, int N, int K, int64_t* out);

typedef struct vog_batch {
  int B, ncmp, T;                      /* T = max sentence length of the batch (host) */
  const int64_t* srl_arg_words_ind;    /* [B,nvl,nsrl,seq_len] */
  const int64_t* srl_arg_word_mask;    /* [B,nvl,seq_len]  (not modified) */
  const int64_t* srl_arg_word_mask_len;/* [B,nvl] */
  const int64_t* srl_arg_words_capture;/* [B,nvl,nsrl,2] */
  const int64_t* srl_arg_inds_msk;     /* [B,nvl,nsrl] */
  const int64_t* num_cmp_msk;          /* [B,ncmp] */
  const int64_t* verb_ind_in_srl;      /* [B,ncmp] (sep) or NULL */
  const float* pad_region_feature;     /* [B,(ncmp,)NP,prop_dim] */
  const float* seg_feature_for_frms;   /* [B,(ncmp,)F,seg_dim] */
  const float* pad_proposals;          /* [B,(ncmp,)NP,7] */
  /* outputs (device, caller-owned) */
  float* mdl_outs; float* mdl_outs_eval;           /* [B,nc_v,nsrl,NP] */
  float* vidf_outs; float* fin_scores_loss; float* fin_scores;  /* sep only */
  void* pred_rec;                                  /* [B] packed records or NULL */
  /* Optional: argument vectors computed elsewhere - vog_lang_forward over a GROUP of batches, or once per checkpoint for the
   * rows of a language bank (engine.py: the vector form `lang_arg_vec` / `lang_final_hidden`, dat_loader_simple.LangBank).
   * shared_lang != NULL: this batch's rows [B*nvl*nsrl, lang_enc] of that output;
   * the language chain is skipped and the four word-level inputs above may be NULL (srl_arg_inds_msk stays).
   * shared_final_hidden: its rows [B*nvl, lang_enc] of the final hidden projection (sep only).
   * With enc_prop or obj_out set as well, the forward's prologue - mul_pl, vis_prep (box-bias precursors only), vis_concat /
   * obj_restore: three launches that read inputs and weights only and write disjoint buffers - is ONE launch, `bank_prep`
   * (csrc/elementwise.hip), where all of these hold: mul_tx's layer 0 is structured, B*nvl*nsrl <= 64 rows with
   * fragment-ordered weights, lang_enc <= 256, 16-byte aligned rows, "pair_launches" on. The three launches stay: on the
   * hi + lo plan (its mul_pl is the split body, up to several launches), beyond 64 argument rows (cfg 5: 80), for models
   * without a structured layer 0 (igrnd / vgrnd, the small test models), with raw features (the group member's sequence,
   * pinned by tests/golden/step_traces.json), with "pair_launches" 0 and when a step is timed on its own. Same bits either way. */
  const float* shared_lang;
  const float* shared_final_hidden;
  /* Optional (round 5): sticky stall counter of this batch's forwards, see vog_lstm_layer_args.fault. Pinned host memory
   * lets the host poll it without synchronising the device. */
  uint32_t* fault;
  /* Optional, sep / svsq models with an object transformer: the output rows of obj_tx's last layer computed elsewhere
   * (vog_ctx_obj_videos), [n_vid * NP, prop_enc + seg_enc] fp32. It comes with enc_seg (the sep head reads the segment
   * encodings) and without enc_prop or raw features, which are not read: no feature cast, no encoder, no obj_tx step runs,
   * one `obj_restore` launch writes the 16-bit copies mul_tx reads and the segment columns of prop_seg, and the fp32 rows
   * are read in place. (It sits in front of `stats`: stats / enc_prop / enc_seg stay the struct's last three members, as the
   * layout test of the encoded inputs pins them. Library and callers are built from this one header; the version stays.) */
  const float* obj_out;
  /* Optional (round 6): two words of pinned host memory, the largest |attention logit| (nats; bits of a non-negative float)
   * the forwards of this batch have seen in obj_tx / mul_tx. Sticky maximum, owned by the host (it may reset it): the
   * run-time check behind the per-checkpoint precision plan (engine.py: a logit scale outside the envelope of the operand
   * precision in use is reported and the plan is raised). Needs pred_rec (the prediction head publishes it). */
  uint32_t* stats;
  /* Optional: visual encodings computed elsewhere (vog_ctx_encode_videos). enc_prop != NULL: rows [rows_obj, prop_enc] fp32 =
   * relu(prop_encoder(row)), enc_seg: [n_vid * F, seg_enc] fp32; the encoder stage is skipped and pad_region_feature /
   * seg_feature_for_frms may be NULL. Both or neither. */
  const float* enc_prop; const float* enc_seg;
} vog_batch;

int64_t vog_workspace_bytes(const vog_ctx* c, int B, int ncmp, int T);
/* zero the parts of a fresh workspace that kernels rely on (V^T key padding,
 * LSTM state padding). Call once per (workspace, shape). */
int vog_workspace_init(const vog_ctx* c, int B, int ncmp, int T, void* ws, size_t ws_bytes,
                       void* stream);
int vog_forward(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, void* stream);

/* The encoder stage of a forward on its own: encode the B_like * ncmp_like videos of one pseudo-batch and write the two column
 * blocks of prop_seg as plain tables, enc_prop_out [rows, prop_enc] and enc_seg_out [rows / nppf0, seg_enc] fp32 with
 * rows = B_like * ncmp_like * nfrm0 * nppf0, in (video, frame, proposal) order - what vog_batch.enc_prop / enc_seg take, and
 * what a bank of encoded rows stores (dat_loader_simple.EncodedBank). prop: [rows, prop_dim], seg: [rows / nppf0, seg_dim]
 * fp32. It runs the very steps vog_forward issues for a batch of that geometry (fused or GEMM form, lean or wide, split-K
 * count, hi + lo operands), so a row's encoding is the bits such a forward computes; the encoders are row-local, so the
 * order of the videos is free. ws: a workspace of vog_workspace_bytes(c, B_like, ncmp_like, 1) bytes. */
int vog_ctx_encode_videos(vog_ctx* c, int B_like, int ncmp_like, const float* prop, const float* seg, float* enc_prop_out,
                          float* enc_seg_out, void* ws, size_t ws_bytes, void* stream);

/* vog_ctx_encode_videos extended by one stage, for models whose obj_tx sees one video at a time (sep / svsq): the boxes' part
 * of the prologue, the encoder stage and the obj_tx stack of a forward of geometry (B_like, ncmp_like), then obj_out
 * [rows, prop_enc + seg_enc] = the stack's fp32 output and enc_seg_out [rows / nppf0, seg_enc] - what vog_batch.obj_out /
 * enc_seg take, and what dat_loader_simple.ObjBank stores. pad_proposals: [rows, 7]. The rows are the bits such a forward
 * computes. The stack's logit maxima of this workspace are folded into the words given to vog_ctx_set_stats, as the
 * prediction head folds a forward's: forwards served from these rows never run obj_tx and would never report its logits. */
int vog_ctx_obj_videos(vog_ctx* c, int B_like, int ncmp_like, const float* prop, const float* seg, const float* pad_proposals,
                       float* obj_out, float* enc_seg_out, void* ws, size_t ws_bytes, void* stream);
/* Does a row of obj_tx's output depend on WHERE its video sits in the batch? The fused encoder-layer tail walks its k-steps
 * in an order rotated by the workgroup's position (txtail_dev.h: 8 consecutive row blocks share one order), so its fp32 sums
 * - hence the rows' last bits - are those of the band of 8 row blocks a row lies in. Returns the rows of one band (8 x 64,
 * 8 x 32 with hi + lo operands), 0 when the rows are position-free (the tail as separate launches), < 0 without obj_tx or
 * before vog_ctx_finalize. Cached rows (vog_batch.obj_out) equal the raw path's bit for bit when the batch has no more rows
 * than one band, or a video is used in the band it was computed in; otherwise they are the bits of another, equally valid
 * summation order. */
int vog_ctx_obj_band_rows(const vog_ctx* c);
/* Two words of pinned host memory (vog_batch.stats of this context's forwards) for the entries that run attention outside a
 * forward; NULL: they publish nothing. */
int vog_ctx_set_stats(vog_ctx* c, uint32_t* stats);

/* named intermediate inside the workspace (parity tests): returns offset/bytes */
int vog_workspace_stage(const vog_ctx* c, int B, int ncmp, int T, const char* stage,
                        int64_t* offset, int64_t* bytes);

/* hipGraph capture of one forward with fixed pointers (launch-bound regime:
 * ~50 launches per batch). Shorthand for vog_graph_capture_desc with nothing but ctx, batch and workspace set. */
typedef struct vog_graph vog_graph;
int vog_graph_capture(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes,
                      void* stream, vog_graph** out);
int vog_graph_launch(vog_graph* g, void* stream);
/* The same graph with the batch's way onto the device in front of the forward ("fed" graph; shorthand for
 * vog_graph_capture_desc with dma, asm_args and the segments set): one host -> device DMA transfer
 * (memcpy node) of dma->bytes if dma != NULL, then vog_assemble_batch(asm_args) if asm_args != NULL, then
 * vog_copy_segments(segs, nseg) if nseg > 0, then the forward - so that a step of a host-fed loop is ONE hipGraphLaunch: the
 * loader writes the next batch into pinned host memory at fixed addresses. Two forms: zero copy (dma == NULL; asm_args' *_in
 * pointers and the segments' sources ARE the pinned host buffer, the kernels read it over the host link: no transfer set-up
 * latency, ~40 GB/s) and DMA (the packed host buffer goes to a device staging buffer first, the kernels read that: the copy
 * engine's ~55 GB/s on large batches). The caller must not rewrite the host buffer before the launch that reads it has
 * completed. */
int vog_graph_capture_fed(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, const vog_copy_seg* dma,
                          const vog_assemble_args* asm_args, const vog_copy_seg* segs, int nseg, void* stream, vog_graph** out);
/* The fed graph with vog_assemble_from_bank(bank_args, required) in place of vog_assemble_batch (shorthand for
 * vog_graph_capture_desc with bank_args in place of asm_args): the staging buffer then holds the
 * batch's video indices and the small word-level arrays only (`bank_args->index` points into it). */
int vog_graph_capture_fed_bank(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, const vog_copy_seg* dma,
                               const vog_bank_assemble_args* bank_args, const vog_copy_seg* segs, int nseg, void* stream,
                               vog_graph** out);
/* The fed graph with the rest of a VALIDATION step behind the forward, on the same linear chain (shorthand for
 * vog_graph_capture_desc without a gather and with epi required): vog_loss_fwd(epi->loss) if
 * given, vog_ground_metrics(epi->metrics) if given, then vog_val_log(epi->log) (required) - a validation step is then one
 * transfer and ONE hipGraphLaunch, and nothing is read back per step. With metrics the log rides in the metrics launch
 * (vog_gmetric_args.log is set to epi->log for the captured call; a separate log launch cost more than the fed loop spreads
 * by); without them vog_val_log is a launch of its own. asm_args / bank_args: at most one of them (neither: the
 * segments alone feed the slot). Every epilogue argument is a fixed address at capture time; per launch only the contents of
 * the buffers change - the batch, and epi->log->step, which one of the segments copies from the staging buffer. */
typedef struct vog_val_epilogue {
  const vog_loss_args* loss;
  const vog_gmetric_args* metrics;
  const vog_val_log_args* log;
} vog_val_epilogue;
int vog_graph_capture_val(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, const vog_copy_seg* dma,
                          const vog_assemble_args* asm_args, const vog_bank_assemble_args* bank_args, const vog_copy_seg* segs,
                          int nseg, const vog_val_epilogue* epi, void* stream, vog_graph** out);
/* The fed graph from a descriptor - the one capture entry the four above are shorthands for: everything
 * vog_graph_capture_val takes, the epilogue optional, plus the query-bank gather.
 * Chain: [transfer] -> vog_gather_rows(gather) if given -> vog_assemble_from_bank(bank_args) | vog_assemble_batch(asm_args) if
 * given -> vog_copy_segments(segs, nseg) if nseg > 0 -> forward -> epilogue if given. The gather comes first: the bank assembly
 * reads index, target_cmp, srl_boxes_in and srl_boxes_lens from buffers the gather has just written, and the video index may
 * itself be a column of the query bank. With the staged keys and the step number as per-batch keys of the gather, nseg is 0
 * and the graph has no more launches than vog_graph_capture_val's. */
typedef struct vog_fed_desc {
  vog_ctx* ctx; const vog_batch* batch; void* ws; size_t ws_bytes;
  const vog_copy_seg* dma;                    /* optional */
  const vog_gather_args* gather;              /* optional */
  const vog_assemble_args* asm_args;          /* at most one of asm_args / bank_args */
  const vog_bank_assemble_args* bank_args;
  const vog_copy_seg* segs; int nseg;
  const vog_val_epilogue* epi;                /* optional */
} vog_fed_desc;
int vog_graph_capture_desc(const vog_fed_desc* d, void* stream, vog_graph** out);
/* Integer options of a context: eight switches and the precision plan (round 6 removed chain_obj_qkv, pair_attn, fused_argvec,
 * fused_pred, qkv_lean and graph_dag with the measured-negative paths behind them: scratch/negatives/r6_pruned/).
 * "tx_split" (default 0; set by engine.py from the checkpoint): hi + lo 16-bit operands, see vog_ctx_split_supported below.
 * "lstm_persistent" (default 1; env VOG_LSTM_PERSISTENT presets it): use vog_bilstm_layer instead
 * of T step launches where vog_bilstm_layer_supported. Its co-residency limit (4 instances) is met
 * automatically on HIP streams (4 hardware queues execute at most 4 kernels at once); set it to 0
 * with GPU_MAX_HW_QUEUES > 4. "lstm_inject_stall": test hook (vog_lstm_layer_args.inject_stall).
 * "lstm_wide" (default 0): with "lstm_persistent" on, a language chain of 17 .. 32 sentences
 * (vog_bilstm_layer_wide_supported) runs one vog_bilstm_layer_wide launch per layer instead of the T step launches; layer 0
 * reads the gate table where the checkpoint has one and Bn * T <= 768, otherwise its input projection stays a GEMM launch, as
 * those of the layers >= 1 do. Such a forward forms no pair launches. "lstm_persistent" = 0 switches it off as well.
 * "fused_tail" (default 1): run everything after the attention of an encoder layer (and, for the
 * last mul_tx layer, lin2 + the score head) as ONE vog_tx_tail_fwd launch where
 * vog_tx_tail_supported (d in {256, 384, 512, 768}); 0 = the separate GEMM / LayerNorm / score launches (always used for other
 * shapes).
 * "fused_enc" (default 1): vog_vis_encode instead of cast + two split-K GEMMs + finish where supported.
 * "enc_lean" (default -1 = the 64-row stream form exactly when the encoders will share a BiLSTM layer's launch; 0 / 1 force).
 * "pair_launches" (default 1): step i of the language chain (input projection / BiLSTM layer / out-projection)
 * and step i of the visual chain (encoders / obj_tx QKV, attention, tail / mul_tx QKV) - independent until
 * mul_tx's attention - share ONE launch (csrc/pair.hip: blocks [0, nA) run one kernel body, the rest the
 * other) wherever a pair kernel exists for the two shapes; 0 = every step its own launch. Same kernel
 * bodies either way: results are bit-identical (tests/test_gpu_forward.py). It also switches `bank_prep`, the one-launch
 * prologue of a forward served entirely from banks (vog_batch.shared_lang). "pair_mask" (default 15): which of the
 * pairs are formed (1 BiLSTM layer 0 + encoders, 2 layer 1 + obj_tx tail, 4 out-projection + mul_tx QKV, 8 (round 6) layer-1 input
 * projection + obj_tx QKV where that projection is a GEMM launch: more than 80 (sentence, position) columns).
 * "fused_ih" (default 1): the BiLSTM input projections run inside the persistent layer kernel
 * (vog_lstm_layer_args.wih) instead of as GEMM launches, where Bn*T <= 80 and K % 256 == 0; round 6: where that prologue
 * does not reach (more than 80 columns: cfg 3, cfg 5, grouped requests) layer 0 reads its gate inputs from the checkpoint's
 * gate table (vog_lstm_layer_args.gx_table, built by vog_ctx_finalize; VOG_GX_TABLE_MAX_MB, default 2048, bounds its size)
 * instead of running a GEMM launch (0: GEMM launches only, 2: layer 0 only, 3: layers >= 1 only, 4: as 1 without the table,
 * 5: the table wherever the checkpoint has one). Measured on MI355X (cfg 2): two launches fewer, W_ih streamed
 * by the layer's 64 CUs (+7 / +17 us per layer against 6.4 / 9.7 us for the whole-chip GEMMs):
 * 43.1 k vs 40.9 k queries/s with 4 batches in flight, 10 us more single-batch latency. */
int vog_ctx_set_int(vog_ctx* c, const char* name, int value);
/* round 6: 1 if the option "tx_split" (hi + lo 16-bit operands: three MFMAs per product for everything that feeds attention
 * logits - encoders, QKV projections, Q.K^T, the tails whose output is another layer's input) has kernels for this model at
 * `ncmp` videos per query: fused encoders, fused tails (d = 512 / 768), structured mul_tx layer 0 and attention whose K ring fits
 * the LDS - the full-size models at 5 or 100 proposals per frame; not the small-dim models, not ImgGrnd. Set the option BEFORE vog_ctx_finalize (the remainder weights are made there). */
int vog_ctx_split_supported(const vog_ctx* c, int ncmp);
int vog_graph_destroy(vog_graph* g);

/* ---- language encoder over a group of batches ------------------------------------------------
 * The BiLSTM re-streams W_hh (16.8 MB per layer) in every one of its 2T dependent step launches:
 * at bs = 4 that is more than half of a forward's HBM traffic, for 4 of the 16 rows of the MFMA
 * tile. vog_lang_forward runs the language chain (mdl_vog.py:250-283 + :97-140) once for the
 * concatenated sentences of several in-flight batches (`lb`: B = sum of the members' B, T = max
 * of their T; the five word-level arrays are the members' arrays back to back, which is how
 * VogEngine.make_group allocates them). Rows never interact (the recurrence, the projections and
 * the argument gather are row-wise), so each member's argument vectors are what its own forward
 * computes up to fp32 summation order. Members then run vog_forward / graphs / AQL programs with
 * vog_batch.shared_lang pointing at their rows of vog_lang_outputs(). */
int64_t vog_lang_workspace_bytes(const vog_ctx* c, int B_total, int ncmp, int T);
int vog_lang_workspace_init(const vog_ctx* c, int B_total, int ncmp, int T, void* lang_ws, size_t bytes, void* stream);
/* lb: only B, ncmp, T and the five srl_* word-level pointers are read */
int vog_lang_forward(vog_ctx* c, const vog_batch* lb, void* lang_ws, size_t bytes, void* stream);
/* LSTMEncoder.forward on its own (replaces /root/reference utils/mdl_srl_utils.py:114-169; SURVEY.md 8(b) `vog_bilstm_fwd`):
 * token re-index (code/mdl_vog.py:67-95) + embedding + the packed 2-layer BiLSTM - both layers, both directions - on a
 * language workspace (vog_lang_workspace_bytes / _init). `lb` as for vog_lang_forward. Outputs, plain fp32 rows:
 * x_out [Bn, T, 2R] (zero past each sentence's length, like pad_packed_sequence) and final_hidden [Bn, 2R] =
 * [h_fwd(last valid step) || h_bwd(first step)] of the top layer (what lang_encode feeds lstm_out_feat_proj,
 * code/mdl_vog.py:262-283). The forward itself never calls this: it keeps the layer output in MFMA operand order for the
 * projection that follows (vog_bilstm_layer x 2 inside vog_forward / vog_lang_forward). */
int vog_bilstm_fwd(vog_ctx* c, const vog_batch* lb, void* lang_ws, size_t bytes, float* x_out, float* final_hidden,
                   void* stream);
/* the conversion at its end: 16-bit layer output (frag = 1: A-fragment order of the M <= 64 GEMM) -> plain fp32 rows */
int vog_lstm_out_to_f32(const void* out16, int frag, int rows_x, int rows_f, int W, vog_dtype dtype, float* x, float* fin,
                        void* stream);
/* device pointers inside lang_ws: argument vectors [B_total*nvl*nsrl, lang_enc] and the final
 * hidden projection [B_total*nvl, lang_enc] */
int vog_lang_outputs(const vog_ctx* c, int B_total, int ncmp, int T, void* lang_ws, float** lang,
                     float** final_hidden);
/* One hipGraph / one AQL program for a whole group: the group's language chain, then every
 * member's remaining forward (members[i].shared_lang must already point into lang_ws).
 * AQL rows: language rows first, then row r of every member behind one barrier packet. */
int vog_group_forward(vog_ctx* c, const vog_batch* lb, void* lang_ws, size_t lang_bytes,
                      const vog_batch* const* members, void* const* workspaces, const size_t* ws_bytes,
                      int n_members, void* stream);
int vog_group_graph_capture(vog_ctx* c, const vog_batch* lb, void* lang_ws, size_t lang_bytes,
                            const vog_batch* const* members, void* const* workspaces,
                            const size_t* ws_bytes, int n_members, void* stream, vog_graph** out);


/* The launches vog_forward would issue for this batch and workspace, one name per line, in issue order
 * (paired launches as "a+b"; nothing is launched). lang_only: the group language chain (vog_lang_forward).
 * Returns 0, or -2 when `out` is too small. */
int vog_describe_steps(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes, int lang_only, char* out, size_t out_bytes);

/* HIP-event timing of `iters` back-to-back launches of ONE hot kernel of the
 * forward on `stream` (bench.py roofline leg). kernel: "mul_qkv", "mul_attn",
 * "mul_wo", "mul_ffn1", "mul_ffn2", "lin2", "obj_qkv", "obj_attn", "prop_enc".
 * Returns average microseconds per launch in *usec. */
int vog_time_kernel(vog_ctx* c, const vog_batch* b, void* ws, size_t ws_bytes,
                    const char* kernel, int iters, void* stream, float* usec);

#ifdef __cplusplus
}
#endif
#endif /* VOG_HIP_H */
