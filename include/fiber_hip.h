/* fiber_hip.h -- C ABI of libfiber_hip.so, the MI355X (gfx950) kernels behind the FIBER coarse-grained
 * fused-backbone forward/backward path.
 *
 * The reference has no FFI: its hot path is Python calling ATen.  Each entry point below replaces the ATen call
 * sequence of one reference function (file:line relative to /root/reference/coarse_grained/fiber/modules/).
 * A maintainer binds them with ctypes (fiber_amd/lib.py is that binding).
 *
 * Conventions: every pointer is a DEVICE pointer; "bf16" buffers are passed as void* (uint16 storage, row-major);
 * fp32 is used for parameters of normalisation/bias, statistics and gradient accumulators; `stream` is a hipStream_t
 * (the caller's current stream -- kernels are stream-ordered, re-entrant, and never synchronise the host);
 * the return value is one of the FIBER_ codes below.
 * Inputs are borrowed and never mutated; outputs and workspaces are caller-allocated.
 *
 * This file is the one statement of the ABI.  csrc/common.h includes it, so the compiler checks every definition against its
 * declaration, and fiber_amd/lib.py derives its ctypes prototypes and constants from it (lib.parse_header).  Keep it in the subset that
 * reader takes: comments, preprocessor lines, `#define FIBER_<NAME> <integer literal>` and one `int|long fiber_<name>(<named parameters>);`
 * per entry point, with scalar parameters of type int, long, long long, unsigned [int], unsigned long long, uint64_t, float or double,
 * and `fiber_stream_t stream` last where the entry point launches.
 */
#ifndef FIBER_HIP_H
#define FIBER_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ihipStream_t* fiber_stream_t;

/* Return value of every entry point that takes a stream: ok; invalid argument (a shape / alignment / pointer contract stated below is
 * violated, nothing was launched); launch failure. */
#define FIBER_OK 0
#define FIBER_EINVAL 1
#define FIBER_ELAUNCH 2
/* Workspace floats of fiber_dot_bf16 and of fiber_stream_add_bwd's d alpha: one partial per workgroup, at most this many workgroups. */
#define FIBER_DOT_PARTS 512

/* The `act` argument of fiber_gemm_nt_bf16: an epilogue mode in the low byte, or-ed with option bits.
 * Modes: 0 none; FIBER_ACT_GELU = exact-erf GELU (Ypre, if non-NULL, gets the pre-activation); FIBER_ACT_GELU_BWD = fused GELU backward. */
#define FIBER_ACT_GELU 1
#define FIBER_ACT_GELU_BWD 2
/* Mode 0 without residual: Y is fp32 [M, ldy] -- narrow outputs whose consumers need more than bf16 (the offset predictor of the
 * deformable convolutions: sampling positions).  Register-staged kernels only. */
#define FIBER_ACT_OUT_F32 0x100
/* Mode 0, residual required: the fp32 RESIDUAL STREAM form of the residual epilogue, described under the prototype. */
#define FIBER_ACT_STREAM_F32 0x800
/* tools/gemm_trace.py: the per-phase timing build of the q8 kernel; `colpart` receives the clock readings. */
#define FIBER_ACT_TRACE 0x1000
/* Set by the entry point itself, callers leave them clear: the output is larger than the last-level cache and is stored non-temporally;
 * keep the two wave groups' stagger across tiles (FIBER_GEMM_STAGGER=1, A/B runs). */
#define FIBER_ACT_NT_STORES 0x2000
#define FIBER_ACT_KEEP_STAGGER 0x4000

/* nn.Linear (+bias, +exact-erf GELU, +per-sample DropPath scale, +residual) : Y = rowscale*act(X.W^T + bias) + R
 * replaces: swin_transformer.py:197,221,233,238,257 (qkv/proj/i2t linears), timm Mlp fc1/fc2 (:325), PatchMerging.reduction
 * (:431), roberta.py:231-241,337,398,415, fiber_module.py:349-350.  act: the FIBER_ACT_ values above.
 * Requires K%8==0, N%4==0, ldx/ldw%8==0, ldy/ldr%4==0. */
/* FIBER_ACT_GELU_BWD: Y = rowscale * (X.W^T) * gelu'(aux) with aux = saved pre-activation [M, ldaux];
 * colpart (nullable) receives per-row-tile column sums of Y, [ceil(M / fiber_gemm_row_tile(M,N,K)), N] fp32 (bias gradient). */
int fiber_gemm_nt_bf16(const void* X, const void* W, const float* bias, const void* residual, void* Y, void* Ypre,
                       const float* rowscale, int rows_per_sample, const void* aux, int ldaux, float* colpart, int M, int N,
                       int K, int ldx, int ldw, int ldy, int ldr, int act, fiber_stream_t stream);
/* FIBER_ACT_STREAM_F32 = the fp32 RESIDUAL STREAM form of the residual epilogue (x = x + branch of
 * swin_transformer.py:388-391, dense + input_tensor of roberta.py:417-423,485 -- the reference keeps these sums in fp32):
 * `residual` is fp32 [M, ldr]; the sum is stored in fp32 at Ypre viewed as float [M, ldy] and, if Y is non-NULL, once more
 * rounded to bf16 at Y (the copy GEMM consumers of the stream read). */
int fiber_gemm_row_tile(int M, int N, int K);

/* Weight (+bias) gradient of nn.Linear: dW[N,K] (fp32, contiguous) = dY[M,lddy]^T . X[M,ldx]; dbias (nullable, fp32[N]) =
 * column sums of dY.  replaces the ATen addmm-backward (TN GEMM + sum(0)) behind every Linear the reference back-propagates
 * through: swin_transformer.py:197,221,233,238,257, timm Mlp (:325), PatchMerging.reduction (:431), PatchEmbed.proj,
 * roberta.py:231-241,337,398,415, fiber_module.py:349-350.  The M reduction is split inside the launch: workspace must hold
 * S*(N*K + N) floats when S = fiber_gemm_tn_splits(M,N,K) > 1 (NULL otherwise).  N%8==0, K%8==0, lddy%8==0, ldx%8==0.
 * DropPath backward (timm 0.4.12 DropPath on the branch, swin_transformer.py:390-391) folded in: row_mask (nullable, fp32
 * [M / rows_per_sample], the per-sample factors in {0, 1/keep}) makes the rows of dropped samples not contribute, `scale` (= 1/keep;
 * 1 without a mask) multiplies dW and dbias.  rows_per_sample % 64 == 0 when a mask is given. */
int fiber_gemm_tn_splits(int M, int N, int K);
int fiber_gemm_tn_bf16(const void* dY, const void* X, float* dW, float* dbias, float* workspace, int M, int N, int K, int lddy,
                       int ldx, const float* row_mask, int rows_per_sample, float scale, fiber_stream_t stream);
/* fiber_gemm_tn_bf16 with its output rows permuted on the way out: row n of dW (entry n of dbias) is written at row_map[n] (int32 [N], a
 * permutation) -- the gradient of a weight whose working copy has its rows in another order (the head-major qkv projection).  The
 * permutation is applied by the fold of the M splits, so `workspace` is needed for every S: max(S, 1) * (N*K + N) floats. */
int fiber_gemm_tn_rowmap_bf16(const void* dY, const void* X, float* dW, float* dbias, float* workspace, int M, int N, int K, int lddy,
                              int ldx, const float* row_mask, int rows_per_sample, float scale, const int* row_map,
                              fiber_stream_t stream);

/* nn.LayerNorm over the last dim (C%8==0, C<=4096); saves mean/rstd.  replaces swin_transformer.py:362,391,244; roberta.py:485,422 */
int fiber_layernorm_fwd_bf16(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows,
                             int C, float eps, fiber_stream_t stream);
int fiber_layernorm_bwd_grid(int rows); /* workspace = grid*8*C floats */
/* dres (nullable): gradient arriving on the residual path of the same x; fused: dx = LN'(dy) + dres */
int fiber_layernorm_bwd_bf16(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                             const void* dres, void* dx, float* dgamma, float* dbeta, float* workspace, int rows, int C,
                             fiber_stream_t stream);

/* The same on the fp32 residual stream.  flags bit 0: x is fp32 [rows, C] (the un-rounded x of swin_transformer.py:362,391 /
 * the LayerNorm input of roberta.py:485,422).  y32 (nullable): the output once more in fp32 -- RoBERTa is post-LN, its LayerNorm
 * output is the next residual.  Gradients (dy, dres, dx) stay bf16. */
int fiber_layernorm_fwd_stream(const void* x, const float* gamma, const float* beta, void* y, float* y32, float* mean, float* rstd,
                               int rows, int C, float eps, int flags, fiber_stream_t stream);
int fiber_layernorm_bwd_stream(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                               const void* dres, void* dx, float* dgamma, float* dbeta, float* workspace, int rows, int C, int flags,
                               fiber_stream_t stream);

/* PatchMerging gather+concat+LayerNorm (swin_transformer.py:411-430): x [B,H*W,C] -> y [B,H*W/4,4C] */
int fiber_patch_merge_ln_fwd_bf16(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int B,
                                  int H, int W, int C, float eps, fiber_stream_t stream);
int fiber_patch_merge_ln_bwd_bf16(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                  void* dx, float* dgamma, float* dbeta, float* workspace, int B, int H, int W, int C,
                                  fiber_stream_t stream);
/* flags bit 0: x is the fp32 residual stream [B,H*W,C]; y, dy, dx stay bf16 */
int fiber_patch_merge_ln_fwd_stream(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int B,
                                    int H, int W, int C, float eps, int flags, fiber_stream_t stream);
int fiber_patch_merge_ln_bwd_stream(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                    void* dx, float* dgamma, float* dbeta, float* workspace, int B, int H, int W, int C, int flags,
                                    fiber_stream_t stream);

/* LayerNorm + Mlp + DropPath + residual of a Swin block as one kernel per direction (csrc/mlp_rows.hip), C in {128, 256}:
 *   y = x + rowscale[row / rows_per_sample] * (fc2(gelu(fc1(LN(x)))) + b2)
 * replaces norm2 -> timm Mlp -> drop_path -> residual add of SwinTransformerBlock.forward (swin_transformer.py:391; Mlp :325,
 * LayerNorm :320).  The LayerNorm's affine part arrives folded into fc1 (w1p = bf16(W1 diag(gamma)) [4C, C], b1p = b1 + W1 beta
 * [4C], fp32); w2p = FA(W2) [C, 4C]; FA(.) = bf16 copy whose K columns are stored in the order "bits 2 and 3 of the index
 * swapped".  The pre-activation stays on chip; g (optional, bf16 [M, 4C]) receives gelu(H) for the backward.  rowscale NULL = no
 * DropPath. */
int fiber_ln_mlp_fwd_bf16(const void* x, const void* w1p, const float* b1p, const void* w2p, const float* b2, const float* rowscale,
                          void* y, void* g, int M, int C, int rows_per_sample, float eps, fiber_stream_t stream);
/* backward from x and dy (the pre-activation is recomputed): dx [M, C] = dy + LayerNorm-backward of the branch gradient, plus the
 * operands of the fc1 weight-gradient GEMM (fiber_gemm_tn_bf16): dh = rowscale (dy W2) gelu'(H) [M, 4C], xhat = (x - mean) rstd
 * [M, C], bf16.  w2tp = bf16(W2^T) [4C, C], w1tp = FA((W1 diag(gamma))^T) [C, 4C]. */
int fiber_ln_mlp_bwd_bf16(const void* x, const void* dy, const void* w1p, const float* b1p, const void* w2tp, const void* w1tp,
                          const float* rowscale, void* dx, void* dh, void* xhat, int M, int C, int rows_per_sample, float eps,
                          fiber_stream_t stream);

/* Swin (shifted) window attention in image-token order: roll + window_partition + WindowAttention self-attn core +
 * window_reverse + roll (swin_transformer.py:99-126, 195-219, 364-387, mask 327-350).  qkv [B*H*W,3C] -> o [B*H*W,C]. */
/* head_major: 0 = reference channel layout [3][heads][32]; 1 = [heads][3][32] (qkv weight rows permuted by the caller);
 * 2 = [heads][q | k v] line layout; 3, 4 = planar probe layouts, 12 x 12 windows only (anything else -> FIBER_EINVAL).
 * lse: B*Hres*Wres*heads fp32 values saved by the forward for the backward of the SAME call shape; its layout is private
 * ([image][head][token] for windows of <= 336 tokens, [token][head] above) -- no other consumer may interpret it. */
int fiber_window_attn_fwd_bf16(const void* qkv, const float* bias_table, void* o, float* lse, int B, int Hres, int Wres, int C,
                               int heads, int ws, int shift, int head_major, fiber_stream_t stream);
int fiber_window_attn_bwd_slices(int n_windows, int heads);
int fiber_window_attn_colsum_rows(int n_windows, int heads, int ws);   /* rows of colsum_ws; 0 = not available for this ws */
/* dqkv_colsum (optional, fp32[3C]) = column sums of dqkv = bias gradient of the qkv nn.Linear (swin_transformer.py:197),
 * produced by the two passes themselves; colsum_ws fp32[colsum_rows*3C].  Pass both or neither (NULL). */
int fiber_window_attn_bwd_bf16(const void* qkv, const float* bias_table, const void* o, const void* dout, const float* lse,
                               void* dqkv, float* dbias_table, float* delta_ws, float* dbias_ws, float* dqkv_colsum,
                               float* colsum_ws, int B, int Hres, int Wres, int C, int heads, int ws, int shift, int head_major,
                               fiber_stream_t stream);

/* Generic MHA core softmax(q.k^T*scale + kmask).v with optional attention-prob dropout: RoBERTa self-attention
 * (roberta.py:256-326), image->text cross-attention (swin_transformer.py:226-256) and text->image cross-attention
 * (roberta.py:272-276).  D in {32,64}.
 * Every dropout-capable entry point takes the 64-bit key as `seed` + an optional DEVICE pointer `seed_base` (key = seed +
 * *seed_base; NULL = seed alone): a captured hipGraph keeps the per-call-site part by value and re-reads the per-step part from
 * device memory on every replay. */
int fiber_mha_fwd_bf16(const void* q, const void* k, const void* v, const float* kmask, void* o, float* lse, int B, int heads,
                       int Lq, int Lk, int D, int ldq, int ldk, int ldv, int ldo, float scale, float p_drop, uint64_t seed,
                       const uint64_t* seed_base, fiber_stream_t stream);
int fiber_mha_bwd_bf16(const void* q, const void* k, const void* v, const float* kmask, const void* o, const void* dout,
                       const float* lse, void* dq, void* dk, void* dv, float* delta_ws, int B, int heads, int Lq, int Lk, int D,
                       int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv, float scale, float p_drop,
                       uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
/* Causal self-attention (text decoder): softmax(q.k^T*scale + kmask[b, j] + (j > i ? -inf : 0)).v.  Arguments as the two above
 * with Lq == Lk = L, 1 <= L <= 64, D in {32,64}; kmask [B, L] additive (-10000 or finfo(fp32).min padding) or NULL.  Key tiles
 * above a query strip's diagonal are skipped.  Dropout keys (row, key) exactly as the non-causal entry points. */
int fiber_mha_causal_fwd_bf16(const void* q, const void* k, const void* v, const float* kmask, void* o, float* lse, int B,
                              int heads, int Lq, int Lk, int D, int ldq, int ldk, int ldv, int ldo, float scale, float p_drop,
                              uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
int fiber_mha_causal_bwd_bf16(const void* q, const void* k, const void* v, const float* kmask, const void* o, const void* dout,
                              const float* lse, void* dq, void* dk, void* dv, float* delta_ws, int B, int heads, int Lq, int Lk,
                              int D, int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv, float scale,
                              float p_drop, uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
/* Single-token attention of a KV-cached caption decoder (csrc/attn_decode.hip): forward only, no dropout, no lse.  D in {32,64}, C = heads*D.
 * fiber_mha_decode_self_bf16: qkv bf16 [N, ldqkv], row n = [q | k | v] of the token at position t; kv_cache bf16 [N slots, Lmax, 2C],
 * [k | v] per position; anc int32 [N, Lmax] or NULL.  Stores row n's k | v to kv_cache[n, t] and writes o[n] = softmax(scale q.K[0..t]).V
 * (o bf16 [N, ldo]), the key and value of position j < t read from slot anc[n, j] (slot n when anc is NULL), position t taken from qkv.
 * A position j <= t whose anc[n, j] lies outside [0, N) is no key (padding under a key mask) and is skipped; anc[n, t] = n otherwise; a row
 * without any key gives 0.  Positions < t are only read, positions > t never (anc[n, j > t] neither); 0 <= t < Lmax <= 64.
 * fiber_mha_decode_cross_bf16: q bf16 [N = G*R, ldq], row n belongs to image n / R, 1 <= R <= 16; kv bf16 [G, Lk, 2C] = [k | v] per image
 * token, Lk >= 1, no mask; o bf16 [N, ldo].  An image's K/V is read once for its R rows; a row's output does not depend on R or on the
 * other rows.
 * D, t >= Lmax, Lmax > 64, R > 16, N % R != 0, a leading dimension that is not a multiple of 8 or narrower than its row, NULL or
 * misaligned (16 bytes; anc: 4) pointers -> 1. */
int fiber_mha_decode_self_bf16(const void* qkv, void* kv_cache, const int* anc, void* o, int N, int heads, int D, int t, int Lmax,
                               int ldqkv, int ldo, float scale, fiber_stream_t stream);
int fiber_mha_decode_cross_bf16(const void* q, const void* kv, void* o, int N, int R, int heads, int Lk, int D, int ldq, int ldo,
                                float scale, fiber_stream_t stream);

/* RobertaEmbeddings.forward (roberta.py:169-199, 877-888) and its backward: dword / dpos rows of the ids / positions present and dtype row 0,
 * dgamma, dbeta are overwritten (the caller zeroes the other table rows), every sum in a fixed order; workspace: the floats
 * fiber_roberta_embed_bwd_workspace returns */
int fiber_roberta_embed_fwd(const int64_t* ids, const float* word, const float* pos_tab, const float* type_tab,
                            const float* gamma, const float* beta, void* y, int* pos_out, float* mean, float* rstd, int B, int S,
                            int C, int pad, float eps, float p_drop, uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
int fiber_roberta_embed_bwd(const void* dy, const int64_t* ids, const int* pos, const float* word, const float* pos_tab,
                            const float* type_tab, const float* gamma, const float* mean, const float* rstd, float* dword,
                            float* dpos, float* dtype, float* dgamma, float* dbeta, float* workspace, int B, int S, int C, int pad,
                            float p_drop, uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
long fiber_roberta_embed_bwd_workspace(int B, int S, int C);

/* timm PatchEmbed Conv2d(3->C,k=4,s=4) as im2col (K=48 ordered [c][kh][kw], zero padded to 64) feeding fiber_gemm_nt_bf16 */
int fiber_im2col_patch4(const float* img, void* cols, int B, int H, int W, fiber_stream_t stream);
/* ... of the 2B-sample batch [img ; where(sel, img, alt)] that the one-pass MLM + ITM step feeds the backbone (objectives.py:56-61 draws
 * the ITM images, :17-75 are the two passes), gathered from the two fp32 sources [B,3,H,W]; sel uint8 [B]. cols bf16 [2B*(H/4)*(W/4), 64]. */
int fiber_im2col_patch4_pair(const float* img, const float* alt, const unsigned char* sel, void* cols, int B, int H, int W,
                             fiber_stream_t stream);

/* element-wise / reduction helpers (n % 8 == 0).  These, the cross-entropy, RoBERTa embedding and im2col entry points refuse (FIBER_EINVAL)
 * a base pointer that their vector accesses would use unaligned: 16 bytes, 8 for the bf16x4 outputs of the embedding and im2col. */
int fiber_gelu_bwd_bf16(const void* dgelu, const void* h_pre, void* dh, long n, fiber_stream_t stream);
int fiber_gelu_bwd_colsum_bf16(const void* dgelu, const void* h_pre, void* dh, float* db, float* workspace, int M, int N,
                               fiber_stream_t stream);
int fiber_scale_add_bf16(const void* a, const void* b, const float* alpha, float mult, void* out, long n, fiber_stream_t stream);
/* out[0] = sum(a*b), overwritten; workspace fp32[512] (NULL allowed when n <= 2048): per-workgroup partials, folded in a fixed order */
int fiber_dot_bf16(const void* a, const void* b, float* out, float* workspace, long n, fiber_stream_t stream);
int fiber_colsum_slabs(int M, int N); /* workspace = slabs*N floats when slabs > 1 */
int fiber_colsum_bf16(const void* x, float* out, float* workspace, int M, int N, int ld, fiber_stream_t stream);
int fiber_fold_rows_f32(const float* part, float* out, int rows, int N, fiber_stream_t stream);
int fiber_dropout_bf16(const void* x, void* y, long n, float p, uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
/* timm 0.4.12 DropPath factors (swin_transformer.py:322,390-391): out[b] = floor(keep + U_b) / keep, fp32 [n] */
int fiber_droppath_scale_f32(float* out, int n, float keep, uint64_t seed, const uint64_t* seed_base, fiber_stream_t stream);
int fiber_rowscale_add_bf16(const void* r, const void* x, const float* scale, void* out, long n, long per_sample,
                            fiber_stream_t stream);
/* Everything the reference does between a branch and its residual, in one pass:
 *   out = res + rowscale[sample] * (drop_a(a) + alpha * drop_b(b))
 * = swin_transformer.py:259 (x + alpha_i2t * y) followed by :390 (shortcut + drop_path(x)); roberta.py:339 / :420 (dense ->
 * dropout -> + input_tensor) and :483-485 (alpha_t2i * cross + self, + hidden_states).  res_kind: 0 none, 1 bf16, 2 fp32 (the fp32
 * residual stream); b, alpha, rowscale nullable; p_a / p_b dropout probabilities (0 = off) with keys seed_a / seed_b (+ *seed_base);
 * out32 (fp32) and / or out16 (bf16), at least one.  n % 8 == 0; per_sample % 8 == 0 when rowscale is given. */
int fiber_stream_add(const void* res, int res_kind, const void* a, const void* b, const float* alpha, const float* rowscale,
                     long per_sample, float p_a, uint64_t seed_a, float p_b, uint64_t seed_b, const uint64_t* seed_base,
                     float* out32, void* out16, long n, fiber_stream_t stream);
/* branch gradients of the above: da, db (nullable), dalpha (nullable fp32 scalar, overwritten; needs b and db) with its per-workgroup
 * partials in workspace fp32[512] (NULL allowed when n <= 2048), folded in a fixed order */
int fiber_stream_add_bwd(const void* dy, const void* b, const float* alpha, const float* rowscale, long per_sample, float p_a,
                         uint64_t seed_a, float p_b, uint64_t seed_b, const uint64_t* seed_base, void* da, void* db, float* dalpha,
                         float* workspace, long n, fiber_stream_t stream);
/* y (bf16) = x (fp32): the bf16 copy of an fp32 stream tensor for a GEMM that consumes it */
int fiber_cast_f32_bf16(const float* x, void* y, long n, fiber_stream_t stream);
/* y = scale[row / rows_per_sample] * x (DropPath backward, swin_transformer.py:390-391) and db = column sums of y (bias
 * gradient of the proj / fc2 linear) in one pass; workspace as for fiber_gelu_bwd_colsum_bf16 */
int fiber_rowscale_colsum_bf16(const void* x, const float* scale, void* y, float* db, float* workspace, int M, int N,
                               int rows_per_sample, fiber_stream_t stream);

/* Cross-entropy over the vocabulary for bf16 logits (caller side: compute_mlm's F.cross_entropy(..., ignore_index=-100),
 * objectives.py:24-28).  fwd: loss[r] = logsumexp(x[r,:]) - x[r, labels[r]] (0 on ignored rows), lse saved; bwd: dlogits =
 * (softmax - onehot) * scale[0] with scale a device scalar (upstream gradient / number of valid rows). */
int fiber_ce_fwd_bf16(const void* logits, const long long* labels, float* loss, float* lse, int* pred, int rows, int V,
                      long long ignore_index, fiber_stream_t stream);
int fiber_ce_bwd_bf16(const void* logits, const long long* labels, const float* lse, const float* scale, void* dlogits, int rows,
                      int V, long long ignore_index, fiber_stream_t stream);
/* pred (nullable, int32 [rows]) of fiber_ce_fwd_bf16: arg max of every labelled row, smallest index among equal maxima as torch.argmax has
 * it, -1 on ignored rows -- the MLM accuracy of the step (gadgets/my_metrics.py:5-28 via fiber_utils.py) without an argmax pass over all rows.
 * fiber_colsum_labelled_bf16: the decoder's bias gradient, column sums of dlogits over the labelled rows only (fiber_ce_bwd_bf16 wrote zeros into
 * the others; heads.py:47-62 MLMHead.bias); workspace fp32 [fiber_colsum_labelled_slabs(rows) * V].  rows above
 * fiber_colsum_labelled_max_rows() are refused with FIBER_EINVAL (a slab's row list would not fit in LDS). */
int fiber_colsum_labelled_slabs(int rows);
int fiber_colsum_labelled_max_rows(void);
int fiber_colsum_labelled_bf16(const void* x, const long long* labels, float* out, float* workspace, int rows, int V,
                               long long ignore_index, fiber_stream_t stream);

/* CIDEr-optimised caption training (caller side: compute_caption_cider, objectives.py:712-896), bf16 logits [rows, V] contiguous, V > 16.
 * fiber_sample_rows_bf16 = objectives.py:756-766 / 781-786 (log_softmax, exp_, torch.multinomial(probs, K, replacement=True), gather): K
 * Gumbel-max draws per row in one read of the row.  tokens[r, k] (int64) = arg max_j (z_j - log(-log(u))), smallest index among equal maxima,
 * u = (hash_u32(seed + *seed_base, (r K + k) V + j) + 0.5) 2^-32, z = the row with column forced_id read as -10000 (:757; forced_id < 0: none);
 * logp[r, k] (fp32) = z_tok - logsumexp(z); ended_out[r, k] (uint8) = tok in {pad_id, sep_id}.  ended (nullable, uint8 [rows]): such a row is not
 * read, its tokens are pad_id, its logp 0, its ended_out 1 (:792).  1 <= K <= 8. */
int fiber_sample_rows_bf16(const void* logits, const unsigned char* ended, long long* tokens, float* logp, unsigned char* ended_out, int rows,
                           int V, int K, int forced_id, uint64_t seed, const uint64_t* seed_base, long long pad_id, long long sep_id,
                           fiber_stream_t stream);
/* objectives.py:818-827 and its autograd (softmax, + 1e-9, log, gather, zero on pad): lp[r] = log(exp(x[r, l] - lse[r]) + 1e-9), l = labels[r];
 * lp = lse = 0 where l == pad_id.  bwd: dlogits[r, j] = rowscale[r] (p_l / (p_l + 1e-9)) ([j == l] - p_j), p = exp(x - lse), rowscale fp32 [rows]
 * in device memory (d loss / d lp[r]); exact zero rows where l == pad_id, so fiber_colsum_labelled_bf16(ignore_index = pad_id) sums the rest. */
int fiber_seqlogp_fwd_bf16(const void* logits, const long long* labels, float* lp, float* lse, int rows, int V, long long pad_id,
                           fiber_stream_t stream);
int fiber_seqlogp_bwd_bf16(const void* logits, const long long* labels, const float* lse, const float* rowscale, void* dlogits, int rows,
                           int V, long long pad_id, fiber_stream_t stream);

/* AdamW step of one parameter group in one launch (caller side of the path: transformers 4.6.0 AdamW(correct_bias=True) as
 * configured by fiber_utils.set_schedule, fiber_utils.py:248-252), also refreshing the bf16 working copies of the weights.
 * table: int64[n*5] device pointers (param fp32, grad fp32, exp_avg, exp_avg_sq, bf16 copy or 0); numel: int64[n];
 * chunks: int32[nchunks*2] (tensor, chunk) pairs of fiber_adamw_chunk() elements; all three in device memory; step >= 1.
 * hyper (nullable): device float[2] {lr, lr*sqrt(1-beta2^step)/(1-beta1^step)} read instead of the by-value lr / step (hipGraph). */
int fiber_adamw_chunk(void);
int fiber_adamw_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks, float lr,
                          float weight_decay, float beta1, float beta2, float eps, int step, const float* hyper,
                          fiber_stream_t stream);
/* All transposed bf16 working copies of the linear weights (the W^T operand of every dX GEMM) in one launch, after the optimizer
 * step -- caller side, next to fiber_adamw_multi_f32 (which rewrites the plain bf16 copies).  table: device array of ndesc 32-byte
 * records {const bf16* src [N,K]; bf16* dst [K,N]; int32 N, K, tile0, tiles_k}; tile0 ascending from 0, a weight owns
 * ceil(N/64)*ceil(K/64) tiles, tiles_k = ceil(K/64); ntiles = the total.  N % 8 == K % 8 == 0. */
int fiber_transpose_multi_bf16(const void* table, int ndesc, int ntiles, fiber_stream_t stream);
/* The grounding solver's optimizer step in three launches (caller side of the fine-grained path): clip_grad_norm_ over every parameter
 * around torch.optim.AdamW with one group per parameter (maskrcnn_benchmark/solver/build.py:8-55), the non-finite skip of GradScaler.step
 * (engine/trainer.py:162-168) and ModelEma.update (utils/ema.py:36-45).  torch's form of the rule: p *= 1 - lr wd first, then
 * p -= lr/(1-beta1^t) m / (sqrt(v)/sqrt(1-beta2^t) + eps).  Tables in device memory: table int64[n*7] device pointers {param fp32, grad fp32,
 * exp_avg, exp_avg_sq, bf16 copy or 0, ema fp32 or 0, coefficient row float[4]}; numel int64[n]; chunks int32[nchunks*2] (tensor, chunk)
 * pairs of fiber_adamw_chunk() elements.
 * fiber_grad_sqnorm_multi_f32: partial[k] (double[nchunks]) = sum of g^2 over chunk k in fp64, fixed order; reads column 1 of the table.
 * fiber_solver_finalize (one workgroup): sum of the partials in index order; norm = sqrt(sum), c = min(1, max_norm / (norm + 1e-6)) in fp64
 * (max_norm = +inf: clipping off).  Non-finite sum: c = 0, skip = 1, skipped_steps += 1, nothing else.  Otherwise steps[i] += 1 (int32[n]) and
 * coef[4 i ..] = {1 - lr wd, lr/(1-beta1^t), 1/sqrt(1-beta2^t), 0} from lr_wd float[n][2], each entry computed in fp64 and rounded once.
 * state: {float norm, float c, int32 skip, int32 skipped_steps}, zeroed once by the caller.
 * fiber_adamw_torch_multi_f32: g' = c g; m' = b1 m + (1-b1) g'; v' = b2 v + (1-b2) g' g'; p' = p decay - s1 m' / (sqrt(v') r2 + eps);
 * copy = bf16(p'); ema' = ema_decay ema + (1 - ema_decay) p' where an EMA pointer is given.  With skip set only the EMA moves (from the
 * unchanged p).  Gradients are never written.
 * fiber_ema_multi_f32: the EMA line alone over table int64[n*2] {src fp32, ema fp32} (entries the optimizer does not step). */
int fiber_grad_sqnorm_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks, double* partial,
                                fiber_stream_t stream);
int fiber_solver_finalize(const double* partial, int npartial, float max_norm, const float* lr_wd, int* steps, float* coef, int n,
                          float beta1, float beta2, void* state, fiber_stream_t stream);
int fiber_adamw_torch_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks, float beta1, float beta2,
                                float eps, float ema_decay, const void* state, fiber_stream_t stream);
int fiber_ema_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks, float decay, fiber_stream_t stream);
/* Row-permuted bf16 working copies (+ their transposes, + the permuted fp32 bias) of fp32 weights in one launch after the optimizer step:
 * the head-major qkv projections of the window-attention blocks (ops._LinearQKVHeadMajor; the permutation is this implementation's, the
 * weights are WindowAttention.qkv, swin_transformer.py:197).  table: device array of ndesc 64-byte records {const float* src [N,K];
 * const int32* perm [N]; bf16* dst [N,K]; bf16* dst_t [K,N] or null; const float* bias [N] or null; float* bias_dst [N]; int32 N, K, tile0,
 * tiles_k}: dst[n] = bf16(src[perm[n]]), dst_t = dst^T, bias_dst[n] = bias[perm[n]]; tiles as in fiber_transpose_multi_bf16. */
int fiber_rowperm_cast_multi_bf16(const void* table, int ndesc, int ntiles, fiber_stream_t stream);
/* On-device input pipeline.
 * fiber_resize_bicubic_norm_u8 replaces transforms/transform.py:10-17 `albef_transform`: torchvision Resize((S,S), BICUBIC) on a
 * PIL RGB image (= Pillow ImagingResample: anti-aliased separable bicubic, 22-bit fixed-point coefficients, 8-bit rounding after
 * each pass) + ToTensor + Normalize, bit-identical to PIL.  descs: device array of n records {int64 src; int32 H, W, src_stride,
 * ksize_h, ksize_v, tmp_off, coef_h_off, coef_v_off} (40 bytes; src = uint8 [H][W][3], ksize_* = fiber_resample_ksize(in, S),
 * offsets into the int32 workspace `coef` (S*(2+ksize) ints per axis and image) and the byte workspace `tmp` (H*S*3 bytes per
 * image)); out: fp32 [n,3,S,S]; max_h = tallest source; mean / std: HOST pointers to 3 floats.
 * fiber_mlm_mask_i64 replaces datamodule_base.py:52 DataCollatorForLanguageModeling.mask_tokens (transformers 4.6.0): tokens with
 * id outside [special_lo, special_hi] are selected with probability p_select / 2^32; selected tokens become labels (others -100)
 * and are replaced by mask_id (80 %), a random id < vocab (10 %) or kept (10 %); draws = counter-based hash of (seed, index). */
int fiber_resample_ksize(int in_size, int out_size);
int fiber_resize_bicubic_norm_u8(const void* descs, int n, int* coef, void* tmp, float* out, int S, int max_h, const float* mean,
                                 const float* std, fiber_stream_t stream);
int fiber_mlm_mask_i64(const long long* ids, long long* ids_mlm, long long* labels, long n, unsigned long long seed,
                       unsigned p_select, int mask_id, int vocab, int special_lo, int special_hi, fiber_stream_t stream);
/* Detection (grounding) input pipeline: the per-sample CPU transforms of the fine-grained model, after the H2D copy of raw bytes.
 * fiber_det_resize_norm_pad_u8 replaces fine_grained/maskrcnn_benchmark/data/transforms/build.py:5-43 `build_transforms` (transforms.py:85-129
 * Resize = PIL Image.resize(BILINEAR) to the per-image Resize.get_size, :131-143 RandomHorizontalFlip, :160-162 ToTensor, :165-177
 * Normalize(format)) and structures/image_list.py:30-72 `to_image_list` (zero padding AFTER normalising), as BatchCollator calls it
 * (data/collate_batch.py:18-21).  Same Pillow ImagingResample as above with the triangle filter (support 1 x max(scale, 1)), bit-identical
 * to PIL.  descs: device array of n records {int64 src; int32 H, W, src_stride, oh, ow, ksize_h, ksize_v, tmp_off, coef_h_off, coef_v_off,
 * flip, tmp_pitch} (56 bytes; ksize_h = fiber_resample_ksize_bilinear(W, ow), ksize_v = (H, oh); `coef` holds ow*(2+ksize_h) +
 * oh*(2+ksize_v) ints per image; `tmp`, 16-byte aligned, holds H*tmp_pitch bytes per image at tmp_off (a multiple of 16), tmp_pitch = 3*ow
 * rounded up to a multiple of 4, plus 16 bytes of slack at its end).  out: fp32 [n,3,Hp,Wp], every element written once: inside (oh, ow)
 * ((v/255 [*255 if times255]) - mean[c]) / std[c] in fp32, each operation rounded, with v read at column ow-1-x when flip and from source
 * channel 2-c when bgr; 0.0f outside.  max_h / max_oh / max_ow: the largest H, oh, ow (oh <= Hp, ow <= Wp).  mean / std: HOST pointers
 * to 3 floats, indexed by output channel.
 * fiber_det_boxes_f32 replaces structures/bounding_box.py:101-135 `BoxList.resize` and :137-171 `BoxList.transpose(FLIP_LEFT_RIGHT)` on the
 * packed targets: boxes fp32 [B,G,4] xyxy in place; params: device array of B records {float ratio_w, ratio_h; int32 flip; float new_w;
 * int32 num_gt} (20 bytes): x *= ratio_w, y *= ratio_h (fp32), then, when flip, (x0, x1) = (new_w - x1 - 1, new_w - x0 - 1); rows
 * g >= num_gt are written as zero. */
int fiber_resample_ksize_bilinear(int in_size, int out_size);
int fiber_det_resize_norm_pad_u8(const void* descs, int n, int* coef, void* tmp, float* out, int Hp, int Wp, int max_h, int max_oh,
                                 int max_ow, int bgr, int times255, const float* mean, const float* std, fiber_stream_t stream);
int fiber_det_boxes_f32(float* boxes, const void* params, int B, int G, fiber_stream_t stream);
/* The coarse-grained model's TRAINING transform, transforms/transform.py:20-45 `albef_transform_randaug`: RandomResizedCrop(BICUBIC) ->
 * RandomHorizontalFlip -> RandomAugment(N, M) (transforms/randaug.py) -> ToTensor -> Normalize.  Every draw is made on the host
 * (data.DeviceRandAugTransform.plan); these entry points execute a plan.
 * fiber_crop_resize_flip_u8 = PIL `img.crop(box).resize((S, S), BICUBIC)` then `transpose(FLIP_LEFT_RIGHT)` where flips[b], bit for bit: the
 * resampler of fiber_resize_bicubic_norm_u8 on a sub-view (descs: the same 40-byte records with src = the box's first pixel, H / W = the
 * box, src_stride = the source's row stride; coef / tmp / max_h as there, for the boxes).  flips: device int32 [n].  out_u8: image b as uint8
 * [S][S][3] at byte b * pitch (pitch >= 3 S^2, a multiple of 16; out_u8 16-byte aligned).  3 kernels.
 * fiber_randaug_slot_u8 = one RandomAugment slot over the batch, 2 kernels whatever the ops are.  slots: device array of n 64-byte records
 * {int32 op, src; float factor; int32 pad; double m[6]}: op = 0 Identity, 1 AutoContrast, 2 Equalize, 3 Brightness, 4 Sharpness, 5 ShearX,
 * 6 ShearY, 7 TranslateX, 8 TranslateY, 9 Rotate, negative = not applied; src = which of buf0 / buf1 (layout of out_u8 above) holds the
 * sample when the slot starts -- the table ops (1-3) run in place, 4-9 write the other buffer; factor: Brightness / Sharpness; m: the
 * inverse affine map of ops 5-9 as cv2.warpAffine inverts it.  luts: uint8 [n][3][256] workspace (the slot's AutoContrast / Equalize /
 * Brightness tables, from the image as it stands when the slot starts).  wtab: int16 [1024][4], cv2's INTER_LINEAR weight table
 * ([fy * 32 + fx][ky * 2 + kx], sum 2^15).  Sharpness keeps the low 8 bits of its truncated fp32 result (the reference's astype(uint8)
 * wraps); the geometric ops follow the generic fixed-point remap path for 8UC3 with constant border 128.  out == NULL: bytes to bytes.
 * out != NULL (the LAST slot): fp32 [n,3,S,S] = (v / 255 - mean[c]) / std[c] as fiber_resize_bicubic_norm_u8 rounds it, and, when out_u8 is
 * not NULL, uint8 [n,S,S,3]: the image before ToTensor.  mean / std: HOST pointers to 3 floats (read when out != NULL). */
int fiber_crop_resize_flip_u8(const void* descs, const int* flips, int n, int* coef, void* tmp, void* out_u8, long long pitch, int S,
                              int max_h, fiber_stream_t stream);
int fiber_randaug_slot_u8(const void* slots, int n, void* buf0, void* buf1, long long pitch, void* luts, const void* wtab, int S,
                          float* out, void* out_u8, const float* mean, const float* std, fiber_stream_t stream);

/* Modulated deformable convolution (DCNv2) of the fine-grained model's DyHead: the sampling half of
 * layers/deform_conv.py:300-353 `ModulatedDeformConv` (csrc/cuda/deform_conv_kernel_cuda.cu:578-640 im2col, :643-700 col2im,
 * :703-773 col2im_coord; host loop csrc/cuda/deform_conv_cuda.cu:497-692).  Channels-last: x bf16 [B,H,W,C], cols / dcols bf16
 * [B*Ho*Wo, kh*kw*C] (tap-major, tap = i*kw + j), offset fp32 [B*Ho*Wo, 2*kh*kw] ((dy,dx) per tap) or NULL, mask fp32
 * [B*Ho*Wo, kh*kw] (after the sigmoid) or NULL; both NULL = ordinary im2col.  The convolution itself is fiber_gemm_nt_bf16 on
 * cols (weights reordered to [Cout, kh*kw*C]); its gradients are fiber_gemm_nt_bf16 / fiber_gemm_tn_bf16.
 * fiber_dcn_scatter_bf16: dx fp32 [B,H,W,C] is accumulated into (caller zeroes; NULL skips), doffset / dmask are written (NULL skips).
 * groups = deformable_groups = 1, dilation 1, C % 8 == 0. */
int fiber_dcn_gather_bf16(const void* x, const float* offset, const float* mask, void* cols, int B, int H, int W, int C, int Ho,
                          int Wo, int kh, int kw, int stride, int pad, fiber_stream_t stream);
int fiber_dcn_scatter_bf16(const void* dcols, const void* x, const float* offset, const float* mask, float* dx, float* doffset,
                           float* dmask, int B, int H, int W, int C, int Ho, int Wo, int kh, int kw, int stride, int pad,
                           fiber_stream_t stream);
/* Input gradient without device atomics (3x3, stride 1 or 2, pad 1, C % 16 == 0): per-tile fixed-point LDS accumulation + a
 * window sum.  dx bf16 [B,H,W,C] is written; workspace = fiber_dcn_dx_workspace() 4-byte words whose LAST B*H*W*C + 4 must be
 * zero on entry. */
long fiber_dcn_dx_workspace(int B, int H, int W, int C, int Ho, int Wo, int stride);
int fiber_dcn_dx_bf16(const void* dcols, const float* offset, const float* mask, void* dx, float* workspace, int B, int H, int W,
                      int C, int Ho, int Wo, int kh, int kw, int stride, int pad, fiber_stream_t stream);

/* Region-word alignment of the grounding head VLDyHead + the binary token focal loss reduced in its epilogue (csrc/ground.hip); file:line
 * relative to /root/reference/fine_grained/maskrcnn_benchmark/.  replaces modeling/rpn/vldyhead.py:857-891 (permute_and_flatten, matmul /
 * log_scale.exp() + bias, clamp to +-50000) and layers/sigmoid_focal_loss.py:130-195 (token_sigmoid_binary_focal_loss, TokenSigmoidFocalLoss
 * .sum()) as called from modeling/rpn/loss.py:1222-1226.
 *   s[b,a,t] = clamp(dot(X[b,a,:], P[b,t,:]) * exp(-log_scale[0]) + tbias[b,t], -50000, 50000)
 * X bf16 [B,A,C] (tower outputs, channels-last, all levels concatenated along A; A arbitrary), P bf16 [B,T,C] (projected tokens), tbias fp32
 * [B,T], log_scale one fp32 in device memory (no host synchronisation).  C = T = 256 only (anything else -> 1).
 * fwd: logits (nullable) fp32 [B,A,T] receives s; loss (nullable, one fp32, overwritten) receives the sum over the tokens with text_mask != 0
 * of alpha_t * softplus(-z) * sigmoid(-z)^gamma, z = +s where target != 0 and -s elsewhere; target uint8 [B,A,T], text_mask uint8 [B,T] (both
 * required with loss); alpha < 0 = no alpha weighting; gamma >= 0.  The loss path writes no [B,A,T] tensor.  At least one output.
 * bwd: recomputes s; with ds = g[0] * dloss/ds (g: upstream scalar in device memory; zero for masked tokens and where the clamp is active):
 * dtbias fp32 [B,T] = sum_a ds, dlog_scale (one fp32) = -sum ds * (s_unclamped - tbias), and `ds` bf16 [B,A,T] receives ds * exp(-log_scale[0]),
 * the gradient of the raw dot product, so that dX = ds . P and dP = ds^T . X are fiber_gemm_nt_bf16 / fiber_gemm_tn_bf16 on it as stored.  workspace: fiber_ground_workspace(B, A, T) floats (per-workgroup partials, folded in a
 * fixed order by fiber_fold_rows_f32; no atomics). */
long fiber_ground_workspace(int B, int A, int T);
int fiber_ground_fwd_bf16(const void* X, const void* P, const float* tbias, const float* log_scale, const unsigned char* target,
                          const unsigned char* text_mask, float* logits, float* loss, float* workspace, int B, int A, int T, int C,
                          float alpha, float gamma, fiber_stream_t stream);
int fiber_ground_bwd_bf16(const void* X, const void* P, const float* tbias, const float* log_scale, const unsigned char* target,
                          const unsigned char* text_mask, const float* g, void* ds, float* dtbias, float* dlog_scale, float* workspace,
                          int B, int A, int T, int C, float alpha, float gamma, fiber_stream_t stream);

/* Grounding inference: VLDyHead's outputs -> boxes with fixed shapes and no host synchronisation (csrc/detect.hip); file:line relative to
 * the reference's fine_grained/maskrcnn_benchmark/.  No atomics: two runs give the same bits.  T = 256 only; NULL or misaligned pointers,
 * C <= 0 and N > fiber_det_max_candidates() -> 1; B == 0 or N == 0 -> 0 without a launch.
 * fiber_det_scores_f32 replaces modeling/rpn/inference.py:620-650 and :741-795 (sigmoid, convert_grounding_to_od_logits[_v2] MEAN / MAX, the
 * candidate test, the centerness product): logits fp32 [B,A,T] and centerness fp32 [B,1,H,W] (= [B,A]) as the head returns them, the positive
 * map as CSR (class_ptr int32 [C+1], tok_idx int32 [nnz], token sets may overlap, an empty class scores 0); out fp32 [B,A,C] =
 * agg * sigmoid(ctr) where agg > pre_nms_thresh (tested BEFORE the centerness product) and -1 elsewhere; agg_max 0 = MEAN, 1 = MAX.
 * fiber_det_scores_rows_f32 is the same with one positive map PER SAMPLE (phrase grounding, referring expressions: a caption per image, which
 * the reference evaluates at batch size 1, engine/inference.py:531): sample b reads its C+1 offsets at class_ptr + b * ptr_stride, absolute
 * offsets into the one shared tok_idx; ptr_stride 0 = fiber_det_scores_f32; 0 < ptr_stride < C+1 -> 1.  A class a sample does not use has an
 * empty row and scores -1.
 * fiber_det_decode_f32 replaces inference.py:657-676, modeling/box_coder.py:52-95 (weights 10,10,5,5, log(1000/16) clamp, TO_REMOVE 1),
 * structures/bounding_box.py:214-225 (clip_to_image) and structures/boxlist_ops.py:77-91 (remove_small_boxes): one level's top-k
 * (topk_val fp32 [B,k], topk_idx int64 [B,k] into [A*C], val < 0 = padding), bbox_reg fp32 [B,4,H,W] read in place, anchors fp32 [A,4],
 * image_sizes fp32 [B,2] (w,h) -> the slice [offset, offset+k) of boxes fp32 [B,N,4], scores (sqrt; -1 for padding and small boxes),
 * labels int32 (c+1), source int32 (level << 28 | a << 10 | c; -1 for padding).  level < 8, A <= 2^18, C <= 2^10.
 * fiber_det_nms_mask replaces csrc/cuda/ml_nms.cu:15-75 (devIoU with the +1 convention in its operation order, label-aware, strict >) on
 * candidates sorted by score: mask uint64 [B,N,ceil(N/64)], bit j of row i set iff j > i, same label, IoU > thresh, both scores >= 0.
 * Only words on or right of the diagonal block are written.
 * fiber_det_nms_select replaces the host loop ml_nms.cu:122-140 and select_over_all_levels inference.py:717-738: walks each image's sorted
 * candidates, stops at D kept; out_boxes fp32 [B,D,4], out_scores [B,D] (-1 past count), out_labels, out_source int32 [B,D], out_count
 * int32 [B].  Deviation: the reference keeps every score >= the kthvalue cut, i.e. more than D on an exact tie at the cut.
 * fiber_det_merge replaces, for chunked evaluation (TEST.CHUNKED_EVALUATION, engine/inference.py:483-575), the concatenation of an image's
 * per-chunk results and data/datasets/evaluation/lvis/lvis_eval.py:137-148 (limit_dets_per_image: sorted(.., reverse=True)[:max_dets]).
 * Inputs are K results per image as fiber_det_nms_select leaves them: boxes fp32 [B,K,D,4], scores fp32 [B,K,D] DESCENDING within each
 * (b,k) over the first count[b,k] slots, labels (chunk-local, 1-based) / source int32 [B,K,D], count int32 [B,K] (clamped to [0,D]; the
 * slots past it are not read as candidates), label_table int32 [K,Cc] (local class c of chunk k -> output label; a label outside 1..Cc
 * reads nothing and yields 0).  Output [B,N,..], N <= K*D: the image's candidates in chunk order then slot order, sorted by descending
 * score, stable (ties: the earlier chunk, then the earlier slot), cut to N; out_chunk int32 [B,N] holds k, out_source is carried
 * unchanged, out_count int32 [B] = min(sum_k count, N); past it box 0, score -1, label 0, source -1, chunk -1.  Every output element
 * is written.  One workgroup per image, the scores in LDS, each candidate's rank by binary searches, a plain scatter: no atomics.
 * K > 64, K*D > fiber_det_merge_max_candidates(), N > K*D, N == 0 with work to do, NULL or misaligned pointers -> 1; B == 0 or
 * K*D == 0 -> 0 without a launch.  NaN scores or lists that do not descend give an unspecified order, never an out-of-bounds access. */
int fiber_det_max_candidates(void);
int fiber_det_merge_max_candidates(void);
int fiber_det_merge(const float* boxes, const float* scores, const int* labels, const int* source, const int* count,
                    const int* label_table, float* out_boxes, float* out_scores, int* out_labels, int* out_source, int* out_chunk,
                    int* out_count, int B, int K, int D, int Cc, int N, fiber_stream_t stream);
int fiber_det_scores_f32(const float* logits, const float* centerness, const int* class_ptr, const int* tok_idx, float* out, int B, int A,
                         int T, int C, float pre_nms_thresh, int agg_max, fiber_stream_t stream);
int fiber_det_scores_rows_f32(const float* logits, const float* centerness, const int* class_ptr, const int* tok_idx, float* out, int B,
                              int A, int T, int C, float pre_nms_thresh, int agg_max, int ptr_stride, fiber_stream_t stream);
int fiber_det_decode_f32(const float* topk_val, const long long* topk_idx, const float* bbox_reg, const float* anchors,
                         const float* image_sizes, float* boxes, float* scores, int* labels, int* source, int B, int k, int A, int C, int N,
                         int offset, int level, float min_size, fiber_stream_t stream);
int fiber_det_nms_mask(const float* boxes, const float* scores, const int* labels, unsigned long long* mask, int B, int N, float nms_thresh,
                       fiber_stream_t stream);
int fiber_det_nms_select(const float* boxes, const float* scores, const int* labels, const int* source, const unsigned long long* mask,
                         float* out_boxes, float* out_scores, int* out_labels, int* out_source, int* out_count, int B, int N, int D,
                         fiber_stream_t stream);

/* Multi-scale test-time augmentation (TEST.USE_MULTISCALE; data/datasets/evaluation/box_aug.py): the merge of the un-cut candidates of up
 * to 24 views of an image, far past the N x N mask of fiber_det_nms_mask.  Fixed shapes, no atomics, no host synchronisation.
 * fiber_det_aug_collect (one launch per view) replaces im_detect_bbox_hflip's BoxList.transpose(0) (structures/bounding_box.py:138-170),
 * remove_boxes (box_aug.py:159-172) and add_preds_t's BoxList.resize (bounding_box.py:102-136), in that order: the view's candidates
 * (boxes fp32 [B,Nv,4] in the resized frame, scores fp32 (< 0 = padding), labels / source int32 [B,Nv]) go to the slots
 * [offset, offset+Nv) of the image's buffers [B,T,..] with `view` beside them.  table: B records {float scaled_w, ratio_w, ratio_h;
 * int32 equal_ratio, flip, has_range; float min2, max2} (32 bytes): when flip, (x1, x2) = (scaled_w - x2 - 1, scaled_w - x1 - 1); when
 * has_range the box lives iff min2 < (x2-x1+1)*(y2-y1+1) < max2, both strict; then x *= ratio_w, y *= (equal_ratio ? ratio_w : ratio_h).
 * classes: ascending int32 [C]; a label outside it, a failed range test and padding are written as box 0, score -1, label 0,
 * source -1, view -1.
 * fiber_det_aug_merge replaces merge_result_from_multi_scales' per-class boxlist_nms (box_aug.py:175-246) for nms_type "nms" (mode 0:
 * greedy, suppress iff IoU > thresh, csrc/cuda/nms.cu:15-23) and "vote" (mode 1: bbox_vote, box_aug.py:249-295: the best remaining
 * candidate and every remaining one with IoU >= thresh TO IT leave as one cluster; a cluster of more than one becomes
 * sum(score * box) / sum(score) in fp32 under the leader's score).  Input: each image's candidates SORTED by (label ascending, score
 * descending), dead slots under a label >= 2^30; classes ascending without repeats; state int32 [B,T] ZEROED by the caller.  One
 * workgroup per (class, image) finds its segment by binary search and loops once per kept box or cluster.  Output: state 1 = kept (its
 * box in out_boxes fp32 [B,T,4], written for kept slots only), 2 = suppressed or merged away, 0 = not of any class in the table.
 * The reduction order is fixed: two runs give the same bits.  thresh <= 0 (no suppression: the caller skips the launch), mode outside
 * {0, 1}, T > fiber_det_aug_max_candidates(), B > 65535, NULL or misaligned pointers -> 1; B, T, Nv or C == 0 -> 0 without a launch.
 * NaN scores or unsorted input give an unspecified result, never an out-of-bounds access. */
int fiber_det_aug_max_candidates(void);
int fiber_det_aug_collect(const float* boxes, const float* scores, const int* labels, const int* source, const void* table,
                          const int* classes, float* out_boxes, float* out_scores, int* out_labels, int* out_source, int* out_view, int B,
                          int Nv, int T, int offset, int view, int C, fiber_stream_t stream);
int fiber_det_aug_merge(const float* boxes, const float* scores, const int* labels, const int* classes, int* state, float* out_boxes,
                        int B, int T, int C, float thresh, int mode, fiber_stream_t stream);

/* Phrase-grounding evaluation (csrc/geval.hip); file:line relative to the reference's fine_grained/maskrcnn_benchmark/.  One wave per
 * (image, phrase); nothing crosses to the host.  fiber_ground_recall replaces engine/inference.py:311-327 (flickr_post_process),
 * data/datasets/evaluation/flickr/flickr_eval.py:173-204 and :365-383 (box_iou, the recall@k tally), data/datasets/refexp.py:58-74
 * (RefExpEvaluator.summarize) and layers/set_loss.py:15-52 (generalized_box_iou).
 * boxes fp32 [B,D,4] in the ORIGINAL image frame, labels int32 [B,D], count int32 [B] (device): the first count[b] rows are read, in their
 * stored descending-score order.  gt fp64 [B,P,G,4]; gt_count int32 [B,P] (0 = no such phrase: hit 0, best 0.0, counted nowhere);
 * cat_mask uint64 [B,P]: the categories the phrase counts towards (bit 0 = "all"), bits >= ncat ignored; topk int32 [K] (device), -1 =
 * every box.  hit int32 [B,P,K], best fp64 [B,P,K]: every element written.  positives / totals int64 [K,64]: ACCUMULATED in place with
 * integer atomic adds (order-independent: two runs give the same bits).
 * mode 0 (Flickr): a detection belongs to phrase p when label == p + 1; its rank is its position among that phrase's detections; one
 * sentinel box [0,0,0,0] follows at the next rank; best[k] = max IoU over ranks < topk[k] and the phrase's gt boxes, IoU in fp64 as
 * inter / (area1 + area2 - inter), no +1; hit = best >= thresh.
 * mode 1 (RefExp): P = 1, labels not read (may be NULL), rank = position, no sentinel; generalized IoU in fp32 of boxes rounded to fp32,
 * compared with thresh rounded to fp32; count[b] == 0: a miss with best = -1 (the reference raises on the empty zip).
 * K > 8, ncat > 64, negative sizes, mode outside {0,1}, mode 1 with P > 1, NULL or misaligned pointers -> 1; B, P or K == 0 -> 0 without
 * a launch. */
int fiber_ground_recall(const float* boxes, const int* labels, const int* count, const double* gt, const int* gt_count,
                        const unsigned long long* cat_mask, const int* topk, int* hit, double* best, long long* positives, long long* totals,
                        int B, int D, int P, int G, int K, int ncat, double thresh, int mode, fiber_stream_t stream);

/* Image-text retrieval evaluation (csrc/retrieval.hip); file:line relative to the reference's coarse_grained/fiber/modules/objectives.py.
 * fiber_retrieval_ranks replaces :361-383 and :477-497 (six topk calls, the id gathers and the recall means) for one score matrix.
 * scores fp32 [Ni,Nt] with row stride ld >= Nt elements (row = image, column = text), iids int32 [Ni], tiids int32 [Nt] (the image id of
 * each caption), ks int32 [nk], nk <= 8.  A query orders its N candidates by descending score, equal scores by ascending candidate
 * index; rank = 0-based position of the first candidate whose id equals the query's, N when none matches; hit@k = rank < k, also for
 * k > N.  Comparisons with NaN are false.  rank_tr int32 [Ni] (an image against the captions), rank_ir int32 [Nt] (a caption against
 * the images), hits int32 [2,nk]: row 0 = image retrieval, row 1 = text retrieval, OVERWRITTEN (zeroed on the stream, then integer
 * atomic adds: two runs give the same bits).  Every element is written.  Two launches, nothing synchronises the host.
 * nk > 8, negative sizes, ld < Nt, NULL or misaligned pointers -> 1. */
int fiber_retrieval_ranks(const float* scores, const int* iids, const int* tiids, const int* ks, int* rank_tr, int* rank_ir, int* hits,
                          int Ni, int Nt, long long ld, int nk, fiber_stream_t stream);

/* Box average precision by the LVIS protocol (csrc/apeval.hip); file:line relative to the reference's
 * fine_grained/maskrcnn_benchmark/data/datasets/evaluation/lvis/lvis_eval.py.  Nothing crosses to the host.
 * fiber_ap_match replaces, for one batch, :137-148 (limit_dets_per_image), :237-241 (the federated filter), :293-317 (compute_iou) and
 * :319-411 (evaluate_img); one wave per (image, area range, threshold).
 * boxes fp32 [B,D,4] xyxy in the ORIGINAL image frame, labels int32 [B,D] (category index + 1), count int32 [B]: the first
 * min(count[b], max_dets) rows are read in their stored descending-score order; max_dets < 0 = no cap.  gt fp64 [B,G,4] xywh, gt_area fp64
 * [B,G] (the annotation's own area), gt_cat int32 [B,G] (category index), gt_ignore uint8 [B,G], gt_count int32 [B]; neg_mask / nel_mask
 * uint64 [B,ceil(C/64)]: bit c = category c is in the image's negative / not-exhaustive list.  iou_thrs fp64 [T] and area_rng fp64 [A,2]
 * are read from device memory as the host computed them.
 * The detection box is x, y, fp32(x2 - x), fp32(y2 - y) (convert_to_xywh, :985-987), everything after it fp64: area w * h,
 * iou = i / (da + ga - i) with i = max(min(dx + dw, gx + gw) - max(dx, gx), 0) * (the same in y) and ga = gw * gh.  A ground truth is
 * ignored when gt_ignore or its area field < lo or > hi; non-ignored ones come first, stable in packing order.  Per (area range,
 * threshold), detections in score order: among unmatched ground truths of the detection's category with iou >= min(thr, 1 - 1e-10) the
 * largest (non-ignored, iou, index) wins.  match / ignore uint64 [B,D]: bit a * T + t; an unmatched detection is ignored when its area is
 * outside the range or its category is not-exhaustive.  valid uint8 [B,D]: 0 past min(count, max_dets), for a label outside 1..C, and when
 * the category is neither among the image's ground truth nor in its negative list (match = ignore = 0 there).  Every element is written.
 * num_gt int64 [C,A]: the non-ignored ground truths, ACCUMULATED in place with integer atomic adds (two runs give the same bits).
 * T * A > 64, G > fiber_ap_max_gt(), negative sizes, NULL or misaligned pointers -> 1; B == 0 -> 0 without a launch.
 * fiber_ap_accumulate replaces :413-524 (accumulate) for all categories at once; one wave per (category, area range, threshold) over
 * chunks of fiber_ap_chunk() records.  match / ignore uint64 [N]: the kept records ordered by category, then by descending score (stable
 * in arrival order); seg_ptr int64 [C + 1] into that order; rec_thrs fp64 [R] ASCENDING.  tp = match & ~ignore, fp = ~match & ~ignore,
 * cumulative integer sums, rc = tp / num_gt, pr = tp / (fp + tp + 2^-52) made non-increasing from the right; precision fp64 [T,R,C,A] = pr
 * at the first index with rc >= rec_thrs[r], 0.0 when there is none; recall fp64 [T,C,A] = the last rc, 0.0 without records; both -1
 * where num_gt == 0.  Every element is written, also with N == 0.  T * A > 64, negative sizes, NULL or misaligned pointers -> 1. */
int fiber_ap_max_gt(void);
int fiber_ap_chunk(void);
int fiber_ap_match(const float* boxes, const int* labels, const int* count, const double* gt, const double* gt_area, const int* gt_cat,
                   const unsigned char* gt_ignore, const int* gt_count, const unsigned long long* neg_mask,
                   const unsigned long long* nel_mask, const double* iou_thrs, const double* area_rng, unsigned long long* match,
                   unsigned long long* ignore, unsigned char* valid, long long* num_gt, int B, int D, int G, int C, int T, int A, int max_dets,
                   fiber_stream_t stream);
int fiber_ap_accumulate(const unsigned long long* match, const unsigned long long* ignore, const long long* seg_ptr, const long long* num_gt,
                        const double* rec_thrs, double* precision, double* recall, long long N, int C, int T, int A, int R,
                        fiber_stream_t stream);

/* Box average precision by the COCO protocol (csrc/apeval.hip): evaluateImg of pycocotools' COCOeval for boxes, which the reference calls
 * at fine_grained/maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py:366-386.  PARITY UNPINNED against the pycocotools binary:
 * the rule below is implemented from its statement.  fiber_ap_accumulate then serves both protocols.
 * fiber_ap_match_coco: one wave per (image, area range, threshold), detections walked in their stored descending-score order.
 * boxes fp32 [B,D,4] xyxy in the ORIGINAL image frame, labels int32 [B,D] (category index + 1), count int32 [B]; gt fp64 [B,G,4] xywh,
 * gt_area fp64 [B,G] (the annotation's own area), gt_cat int32 [B,G], gt_crowd uint8 [B,G] (iscrowd), gt_count int32 [B]; iou_thrs fp64
 * [T], area_rng fp64 [A,2].  There are no federated lists: every category is evaluated in every image.
 * rank int32 [B,D]: the number of earlier slots d' < d < min(count, D) of the image with the same label, for a label in 1..C; -1 for a
 * slot past min(count, D) or a label outside 1..C.  valid uint8 [B,D]: 1 iff rank is in 0..cap-1 (cap = maxDets[-1]: only the first cap
 * detections of an (image, category) exist; a later one is skipped at every (area range, threshold), match = ignore = 0).
 * The detection box is x, y, fp32(x2 - x), fp32(y2 - y), with plus_one = 1 each extent then + 1 in fp32 (prepare_for_coco_detection,
 * :125-154: BoxList.convert("xywh") adds TO_REMOVE, structures/bounding_box.py:79-81); plus_one = 0 for true xywh extents.  Everything
 * after it fp64: da = w * h, iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise, i = 0 if iw <= 0 or ih <= 0 else iw * ih;
 * iou = i / da against a crowd ground truth, i / (da + gw * gh - i) otherwise.  A ground truth is ignored when it is crowd or its area
 * field < lo or > hi.  Per (area range, threshold), detections in score order: among the ground truths of the detection's category with
 * iou >= min(thr, 1 - 1e-10) that are unmatched or crowd, the largest (non-ignored, iou, index) wins; a crowd one is never consumed.
 * match / ignore uint64 [B,D]: bit a * T + t; a matched detection is ignored iff its ground truth is, an unmatched one iff its own area
 * is outside the range.  num_gt int64 [C,A]: the non-ignored ground truths, ACCUMULATED in place with integer atomic adds (two runs give
 * the same bits).  Every element of match, ignore, rank and valid is written.  The ranks are counted in LDS, one counter per category:
 * C > fiber_ap_coco_max_categories() -> 1.  T * A > 64, G > fiber_ap_max_gt(), negative sizes or cap, plus_one outside {0,1}, NULL or
 * misaligned pointers -> 1; B == 0 -> 0 without a launch. */
int fiber_ap_coco_max_categories(void);
int fiber_ap_match_coco(const float* boxes, const int* labels, const int* count, const double* gt, const double* gt_area, const int* gt_cat,
                        const unsigned char* gt_crowd, const int* gt_count, const double* iou_thrs, const double* area_rng,
                        unsigned long long* match, unsigned long long* ignore, int* rank, unsigned char* valid, long long* num_gt, int B,
                        int D, int G, int C, int T, int A, int cap, int plus_one, fiber_stream_t stream);

/* Grounding training: ATSS target assignment and the box / centerness losses with fixed shapes and no host synchronisation
 * (csrc/atss.hip); file:line relative to the reference's fine_grained/maskrcnn_benchmark/.  Targets: gt_boxes fp32 [B,Gmax,4] (xyxy),
 * gt_labels int32 [B,Gmax], num_gt int32 [B], positive_map uint8 [B,Gmax,T]; rows g >= num_gt[b] are never read.  anchors fp32 [A,4]: the
 * levels concatenated in level order; level_off: HOST array of L + 1 anchor offsets (L <= 8, level_off[0] = 0, level_off[L] = A).
 * K = sum_l min(topk, A_l) candidates per gt = fiber_atss_num_candidates (-1 if refused).  NULL or misaligned pointers, T != 256,
 * K < 2 (the reference's unbiased std is NaN) and K > 128 -> 1; B == 0 -> 0 without a launch.  The only atomics are integer (a 64-bit
 * max, a count): two runs give the same bits.
 * fiber_atss_candidates_f32 replaces modeling/rpn/loss.py:697-719 and structures/boxlist_ops.py:96-135 (the [A,G] IoU and distance
 * matrices and the per-level topk): per live (image, gt) and level the min(topk, A_l) anchors nearest to the gt centre by
 * sqrt(dx^2 + dy^2), EQUAL DISTANCES TO THE LOWEST ANCHOR INDEX, in ascending (distance, index) order -> cand_idx int32 [B,Gmax,K]
 * (index into the concatenated anchors) and cand_iou fp32 [B,Gmax,K] (+1 convention).
 * fiber_atss_resolve_f32 replaces loss.py:721-755: threshold mean + unbiased std of the gt's K IoUs (summed in a fixed order),
 * positive = iou >= threshold and min(l,t,r,b) > 0.01 of the anchor centre in the gt; key uint64 [B,A] (zeroed here) receives the maximum
 * over the anchor's positive gts of (iou bits << 32 | 0xFFFFFFFF - g): highest IoU wins, EQUAL IoU TO THE LOWEST GT INDEX; 0 = unassigned.
 * fiber_atss_finalize_f32 replaces loss.py:756-804 and modeling/box_coder.py:22-50 (encode, weights 10,10,5,5): matched int32 [B,A]
 * (-1 unassigned), labels int32 [B,A] (0), reg_targets fp32 [B,A,4] (0), token_targets uint8 [B,A,T] (the matched gt's positive_map row;
 * unassigned: the one-hot on token T-1), num_pos int32 [B] = anchors with labels > 0.
 * fiber_atss_loss_fwd_f32 / _bwd_f32 replace loss.py:583-624 (GIoULoss), :829-844 (compute_centerness_targets), BCEWithLogitsLoss(sum),
 * the pos_inds gathers (:1194, :1237-1254), box_coder.py:52-95 (decode, log(1000/16) clamp) and concat_box_prediction_layers for ONE
 * level: bbox_reg fp32 [B,4,H,W] and centerness fp32 [B,1,H,W] read in place (A_level = H*W anchors at `offset` of the concatenation),
 * dense over the anchors and masked by labels > 0.  fwd: part[(row0 + i)*3 + {0,1,2}], i < fiber_atss_loss_rows(B, A_level), receive
 * per-workgroup sums of w (1 - giou), w and BCE(centerness, w), w the centerness target, to be folded by fiber_fold_rows_f32;
 * ctr_targets (nullable) fp32 [B,A] receives w (0 unassigned) in the level's slice.  bwd: g = three upstream gradients (of the three
 * sums) in device memory; d_bbox_reg [B,4,H,W] and d_centerness [B,1,H,W] are written in full, zeros on unassigned anchors and on a
 * clamped coordinate; max / min ties split the gradient in halves and the clamp passes it at equality, as torch does. */
int fiber_atss_num_candidates(const int* level_off, int L, int topk);
int fiber_atss_candidates_f32(const float* anchors, const int* level_off, int L, const float* gt_boxes, const int* num_gt, int* cand_idx,
                              float* cand_iou, int B, int Gmax, int A, int topk, fiber_stream_t stream);
int fiber_atss_resolve_f32(const float* anchors, const float* gt_boxes, const int* num_gt, const int* cand_idx, const float* cand_iou,
                           unsigned long long* key, int B, int Gmax, int A, int K, fiber_stream_t stream);
int fiber_atss_finalize_f32(const float* anchors, const float* gt_boxes, const int* gt_labels, const unsigned char* positive_map,
                            const unsigned long long* key, int* matched, int* labels, float* reg_targets, unsigned char* token_targets,
                            int* num_pos, int B, int Gmax, int A, int T, fiber_stream_t stream);
int fiber_atss_loss_rows(int B, int A_level);
int fiber_atss_loss_fwd_f32(const float* bbox_reg, const float* centerness, const float* anchors, const int* labels,
                            const float* reg_targets, float* part, float* ctr_targets, int B, int A, int A_level, int offset, int row0,
                            fiber_stream_t stream);
int fiber_atss_loss_bwd_f32(const float* bbox_reg, const float* centerness, const float* anchors, const int* labels,
                            const float* reg_targets, const float* g, float* d_bbox_reg, float* d_centerness, int B, int A, int A_level,
                            int offset, fiber_stream_t stream);

/* FPN top-down pathway of the fine-grained neck (csrc/fpn.hip); file:line relative to the reference's fine_grained/maskrcnn_benchmark/.
 * Channels-last bf16 maps [B,H,W,C], fp32 arithmetic, C % 8 == 0 (16-byte accesses; any other C -> 1).  No floating-point atomics and
 * every output element written exactly once: two runs give the same bits.  Nothing synchronises the host.
 * Nearest index rule of all three: src = min((int)floorf(dst * ((float)Hc / (float)H)), Hc - 1) and the same for W, the scale formed in
 * fp32 -- F.interpolate(mode="nearest", size=...).  (The exact rational dst * Hc / H differs, first at H = 58, Hc = 30.)
 * fiber_dropblock_mask_u8 replaces layers/dropblock.py:45-48 (host torch.rand, the copy) and :61-74 (max_pool2d block mask) and the
 * block_mask.sum() of :57: seeds uint8 [B,H,W] in/out; draw != 0 first sets seeds[i] = hash_u32(seed + *seed_base, i) < (uint32)(gamma *
 * 2^32) (i the flat index; seed by value + optional DEVICE base as fiber_dropout_bf16, so a captured graph draws anew on every replay),
 * draw == 0 reads seeds as given; keep uint8 [B,H,W] = 1 - maxpool_{block x block, stride 1, pad block/2}(seeds); kept int32[1] = sum keep,
 * overwritten (integer accumulation).  block odd (even -> 1), 0 <= gamma < 1.
 * fiber_fpn_merge_fwd_bf16 replaces modeling/backbone/fpn.py:97-108 and dropblock.py:54-57: s = f32(lateral) + f32(coarse[src]),
 * inner_out = bf16(s), dropped_out (nullable, with keep and kept) = bf16(s * keep * scale), scale = (float)(B*H*W) / (float)kept[0] read
 * from device memory and applied to the UNROUNDED sum.  kept[0] == 0 gives what IEEE gives (NaN where keep is 0 -- everywhere), as the
 * reference.  coarse [B,Hc,Wc,C]; Hc == H and Wc == W is the plain add (fpn.py:100-101); coarse NULL: s = f32(lateral) (DropBlock2D alone).
 * fiber_fpn_merge_bwd_bf16 is the backward of it in ONE launch: g = f32(d_inner) + f32(d_dropped) * keep * scale (a NULL term is absent;
 * d_dropped needs keep and kept), d_lateral_out = bf16(g), d_coarse_out[b,hc,wc,:] = bf16(sum of the unrounded g over the fine pixels whose
 * src is (hc,wc), in fp32, row-major child order; 0 where a coarse pixel has no child).  The children are found with the forward rule
 * itself.  d_coarse_out NULL: not written (Hc, Wc ignored). */
int fiber_dropblock_mask_u8(unsigned char* seeds, int draw, uint64_t seed, const uint64_t* seed_base, float gamma, int block,
                            unsigned char* keep, int* kept, int B, int H, int W, fiber_stream_t stream);
int fiber_fpn_merge_fwd_bf16(const void* lateral, const void* coarse, const unsigned char* keep, const int* kept, void* inner_out,
                             void* dropped_out, int B, int H, int W, int C, int Hc, int Wc, fiber_stream_t stream);
int fiber_fpn_merge_bwd_bf16(const void* d_inner, const void* d_dropped, const unsigned char* keep, const int* kept, void* d_lateral_out,
                             void* d_coarse_out, int B, int H, int W, int C, int Hc, int Wc, fiber_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
