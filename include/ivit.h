/* libivit_hip — C ABI of the MI355X-native IntentNetViT hot path (gfx950 / CDNA4).
 *
 * Every entry point is stream-ordered and stateless: buffers are caller-owned device
 * pointers (PyTorch caching allocator on the Python side), sizes are plain integers,
 * the stream is a hipStream_t passed as void*. Return value: 0 on success, <0 for bad
 * arguments (message in ivit_last_error()), >0 for a hipError_t from the launch.
 * dtype selects the compute path: IVIT_F32 (exact f32 MFMA; the parity path) or
 * IVIT_BF16 (bf16 MFMA, f32 accumulation; the throughput path).
 *
 * Each function names the reference interface (file:line under the reference repo) whose
 * arithmetic it implements; the Python host layer mirrors those interfaces.
 */
#ifndef IVIT_H
#define IVIT_H
#ifdef __cplusplus
extern "C" {
#endif

#define IVIT_OK 0
#define IVIT_ERR_ARG (-1)
#define IVIT_ERR_UNSUPPORTED (-2)

#define IVIT_F32 0
#define IVIT_BF16 1

#define IVIT_ACT_NONE 0
#define IVIT_ACT_GELU 1
#define IVIT_ACT_RELU 2
#define IVIT_ACT_GELU_D 3 /* ivit_linear_fwd_panel only: GELU, second output = GELU'(pre-activation) */

/* Tuning knobs (no effect on results; process-wide; defaults from the environment variable named,
 * read once when the library loads):
 *   IVIT_KNOB_WIDE_EPI   (IVIT_WIDE_EPI, default 0): epilogue form of the wide row-panel kernels —
 *                        0 the LDS-tile form for every epilogue, 1 transposed accumulators for the
 *                        Q-prescale and GELU + GELU' outputs, 2 transposed for all;
 *   IVIT_KNOB_CONV_PANEL (IVIT_CONV_PANEL, default 1): 0 runs the stride-1 bf16 convolutions on the
 *                        128 x 128 engine instead of the panel kernels (the tests compare the two);
 *   IVIT_KNOB_DROP_SKIP  (IVIT_DROP_SKIP, default 1): 0 makes the *_skip entry points ignore their
 *                        skip pointer (the DropPath row skip off: every sample is computed). */
#define IVIT_KNOB_WIDE_EPI 0
#define IVIT_KNOB_CONV_PANEL 1
#define IVIT_KNOB_DROP_SKIP 2
#define IVIT_KNOB_COUNT 3

const char* ivit_version(void);
const char* ivit_last_error(void);
int ivit_set_knob(int knob, int value);
long ivit_get_knob(int knob);

/* ---- Linear layers: timm Attention.qkv/proj, Mlp.fc1/fc2 (reached from model_vit.py:64,71,119)
 *      and the adapters nn.Linear(384,192) (model_vit.py:82-83).                              */
/* Y[M,N] = act(X[M,K] W[N,K]^T + b)  (Ypre: optional pre-activation copy), or, when resid != 0,
 * Y(f32) = resid + row_scale[m / rows_per_scale] * (X W^T + b)   (residual + DropPath, timm Block). */
int ivit_linear_fwd(int dtype, const void* X, long ldx, const void* W, const float* bias, long M, long N, long K,
                    int act, void* Y, long ldy, int y_dtype, void* Ypre, const float* resid, long ldr,
                    const float* row_scale, long rows_per_scale, void* stream);
/* Y = X W^T + bias with columns n < scale_cols multiplied by col_scale (after the bias): the
 * fused qkv projection of timm Attention (attn.qkv, timm Attention.forward) writing its Q block
 * pre-multiplied by log2(e)/sqrt(Dh) for ivit_attn_fwd_q2 / ivit_attn_bwd_q2. */
int ivit_linear_fwd_qs(int dtype, const void* X, long ldx, const void* W, const float* bias, long M, long N, long K,
                       void* Y, long ldy, int y_dtype, long scale_cols, float col_scale, void* stream);
/* dX[M,K] = dY[M,N] W[N,K]  (optionally * gelu'(pre[M,K])). */
int ivit_linear_dgrad(int dtype, const void* dY, long lddy, const void* W, long M, long N, long K, void* dX,
                      long lddx, int dx_dtype, const void* gelu_pre, long ldpre, void* stream);
/* dW[N,K] (+)= dY^T X ; dbias[N] (+)= colsum(dY). f32 outputs; split-K through `work`. */
long ivit_linear_wgrad_workspace(long M, long N, long K);
int ivit_linear_wgrad(int dtype, const void* dY, long lddy, const void* X, long ldx, long M, long N, long K,
                      float* dW, float* dbias, int accumulate, void* work, long work_bytes, void* stream);
/* Residual GEMM + the following LayerNorm in one kernel (timm Block: x1 = x + dp1(proj(.)), then
 * norm2(x1); model_vit.py:64,71 -> timm Block.forward), bf16 operands, N = 384:
 *   X = R + scale[m / rps] * (A W^T + bias)  (f32)   Y = bf16(LN(X; gamma, beta, eps)), mean, rstd [M]
 * W packed by ivit_patch_weight_pack(W f32 [N][K], N, K / 64, ...); K % 64 == 0; scale may be null. */
int ivit_linear_resid_ln_fwd(const void* A, long lda, long M, long N, long K, const void* wpack, const float* bias,
                             const float* R, long ldr, const float* scale, long rps, const float* gamma,
                             const float* beta, float eps, float* X, long ldx, void* Y, long ldy, float* mean,
                             float* rstd, void* stream);

/* Backward twin: the LayerNorm input's dgrad with the LayerNorm backward in the epilogue (timm
 * norm1 / norm2 backward after Attention.qkv / Mlp.fc1 dgrad), N = 384, bf16 dY [M][K]:
 *   G = dY W (W [K][N], packed transposed by ivit_weight_pack_t);  dX = dres + LN_bwd(G; X, gamma,
 *   mean, rstd);  dXs = bf16(dX * scale[m / rps]) if non-null;  dgamma / dbeta (+)= column sums.
 * dX may alias dres; work >= ivit_linear_dgrad_ln_bwd_workspace(M, N). */
long ivit_linear_dgrad_ln_bwd_workspace(long M, long N);
int ivit_linear_dgrad_ln_bwd(const void* dY, long lddy, long M, long N, long K, const void* wpack_t, const float* X,
                             long ldx, const float* gamma, const float* mean, const float* rstd, const float* dres,
                             long ldr, float* dX, long lddx, void* dXs, const float* scale, long rps, float* dgamma,
                             float* dbeta, int accumulate, void* work, long work_bytes, void* stream);
/* Row-panel forms of the wide token GEMMs (bf16, N a multiple of 384, K of 64): each workgroup
 * writes one 144-row x 192-column block (two workgroups per CU) (timm Attention.qkv, Mlp.fc1).
 *   act NONE: Y = (A W^T + bias), columns n < qcols times qscale (qkv with the Q block prescaled)
 *   act GELU: Ypre = A W^T + bias (if non-null), Y = gelu(Ypre)   (W packed by ivit_patch_weight_pack) */
int ivit_linear_fwd_panel(const void* A, long lda, long M, long N, long K, const void* wpack, const float* bias,
                          int act, long qcols, float qscale, void* Y, long ldy, void* Ypre, long ldpre, void* stream);
/*   act GELU_D: Ypre = gelu'(A W^T + bias) (if non-null), Y = gelu(A W^T + bias): the derivative
 *   the backward needs, from the f32 pre-activation, instead of the pre-activation itself.
 * dX[M,N] = (dY[M,K] W[K,N]) * gelu'(pre[M,N])  (Mlp.fc2 dgrad into fc1's pre-activation; W packed
 * transposed by ivit_weight_pack_t), bf16. */
int ivit_linear_dgrad_gelu_panel(const void* dY, long lddy, long M, long N, long K, const void* wpack_t,
                                 const void* pre, long ldpre, void* dX, long lddx, void* stream);
/* dX[M,N] = (dY[M,K] W[K,N]) * G[M,N]  (bf16; G = the GELU' that ivit_linear_fwd_panel wrote with
 * act GELU_D: the same fc2 dgrad with no GELU' evaluation in its epilogue). */
int ivit_linear_dgrad_mul_panel(const void* dY, long lddy, long M, long N, long K, const void* wpack_t, const void* G,
                                long ldg, void* dX, long lddx, void* stream);
/* DropPath row skip (timm Block: x + drop_path(branch), per-sample factor in {0, 1/(1-p)}): the four
 * entry points above with `skip`, the factors [ceil(M / rps)] of the branch THIS GEMM belongs to
 * (rps rows per sample, rps > 0). A 144-row panel whose rows all belong to samples with
 * skip[b] == 0 is not computed: the wide kernels store zeros to its rows of Y (and of Ypre where
 * they write one) — zeros, not unwritten rows, because the weight gradient and panels that
 * straddle a kept sample still read them against an exact zero; the LayerNorm kernels run their
 * epilogue on a zero accumulator (X, Y, mean, rstd / dX, dXs and the dgamma / dbeta sums are
 * produced for every row). Results equal the plain entry points' up to the sign of an exact zero,
 * provided the skipped products were finite (a NaN inside a dropped branch no longer spreads).
 * skip == null, or IVIT_KNOB_DROP_SKIP at 0: exactly the plain entry point (which forwards here).
 * ivit_linear_resid_ln_fwd_skip: skip is normally the same pointer as scale;
 * ivit_linear_dgrad_ln_bwd_skip: scale stays the OUTPUT factor of dXs (the hand-off to the
 * previous branch), skip is the branch of dY. */
int ivit_linear_resid_ln_fwd_skip(const void* A, long lda, long M, long N, long K, const void* wpack,
                                  const float* bias, const float* R, long ldr, const float* scale, long rps,
                                  const float* gamma, const float* beta, float eps, float* X, long ldx, void* Y,
                                  long ldy, float* mean, float* rstd, const float* skip, void* stream);
int ivit_linear_dgrad_ln_bwd_skip(const void* dY, long lddy, long M, long N, long K, const void* wpack_t,
                                  const float* X, long ldx, const float* gamma, const float* mean, const float* rstd,
                                  const float* dres, long ldr, float* dX, long lddx, void* dXs, const float* scale,
                                  long rps, float* dgamma, float* dbeta, int accumulate, void* work, long work_bytes,
                                  const float* skip, void* stream);
int ivit_linear_fwd_panel_skip(const void* A, long lda, long M, long N, long K, const void* wpack, const float* bias,
                               int act, long qcols, float qscale, void* Y, long ldy, void* Ypre, long ldpre,
                               const float* skip, long rps, void* stream);
int ivit_linear_dgrad_mul_panel_skip(const void* dY, long lddy, long M, long N, long K, const void* wpack_t,
                                     const void* G, long ldg, void* dX, long lddx, const float* skip, long rps,
                                     void* stream);
/* The weight and bias gradients of one timm Block's four linears (Mlp.fc2, Mlp.fc1, Attention.proj,
 * Attention.qkv; model_vit.py:64,71 -> timm Block backward) in one grouped launch + one reduce:
 *   dW_g = dY_g^T X_g (f32 [N][K]), db_g = colsum(dY_g) (f32 [N], may be null), bf16 token-major
 *   operands [M][*], for (dY, X) = (dy2 [M][D], a [M][Hd]), (dh [M][Hd], x2 [M][D]),
 *   (dyp [M][D], o [M][D]), (dyq [M][3D], x1 [M][D]). D = 384, Hd % 384 == 0, operands 16-B aligned. */
long ivit_vit_block_wgrad_workspace(long M, long D, long Hd);
int ivit_vit_block_wgrad(long M, long D, long Hd, const void* dy2, const void* a, const void* dh, const void* x2,
                         const void* dyp, const void* o, const void* dyq, const void* x1, float* dw2, float* db2,
                         float* dw1, float* db1, float* dwp, float* dbp, float* dwq, float* dbq, void* work,
                         long work_bytes, void* stream);
/* W [K][N] f32 -> the row-panel packed bf16 layout of W^T (ivit_patch_weight_pack_bytes(N, K / 64) bytes). */
int ivit_weight_pack_t(const float* w, long K, long N, void* wpack, void* stream);
/* Many packs in one launch: jobs = device array of n records {const float* w; void* wpack; long rows;
 * long cols; int transposed (+4 pad)} (40 B each); transposed 0 = ivit_patch_weight_pack(w, rows,
 * cols / 64), 1 = ivit_weight_pack_t(w, rows, cols); max_rows_cols >= every rows * cols. */
int ivit_weight_pack_multi(long n, const void* jobs, long max_rows_cols, void* stream);
/* ---- timm PatchEmbed (Conv2d k=s=8) + CLS concat + pos_embed (model_vit.py:64,71 → timm). */
int ivit_patch_embed_fwd(int dtype, const float* img, long B, long C, long H, long W, const void* Wt,
                         const float* bias, const float* pos, const float* cls, long D, float* out, void* stream);
long ivit_patch_embed_wgrad_workspace(long B, long C, long H, long W, long D);
int ivit_patch_embed_wgrad(int dtype, const void* dtok, const float* img, long B, long C, long H, long W, long D,
                           float* dW, float* dbias, float* dpos, float* dcls, int accumulate, void* work,
                           long work_bytes, void* stream);
/* bf16 throughput path of the same PatchEmbed: one coalesced pass over the f32 raster writes the
 * bf16 patch matrix cols[b*Np + gy*Wp + gx][(c*8 + ky)*8 + kx] = img[b][c][8gy+ky][8gx+kx]
 * (full 128-B rows per (patch, channel)); the forward and the weight gradient then stream it
 * as dense GEMM operands by LDS-DMA instead of re-gathering the raster. Same outputs and
 * workspace as ivit_patch_embed_fwd / _wgrad with dtype IVIT_BF16.                          */
int ivit_patch_im2col(const float* img, long B, long C, long H, long W, void* cols, void* stream);
int ivit_patch_embed_fwd_cols(const void* cols, long B, long C, long H, long W, const void* Wt, const float* bias,
                              const float* pos, const float* cls, long D, float* out, void* stream);
int ivit_patch_embed_wgrad_cols(const void* dtok, const void* cols, long B, long C, long H, long W, long D,
                                float* dW, float* dbias, float* dpos, float* dcls, int accumulate, void* work,
                                long work_bytes, void* stream);
/* Fused bf16 forward of the same PatchEmbed: the f32 raster streams through LDS once (converted to
 * bf16 in the operand read), every workgroup computing all D columns of 144 patches; no patch
 * matrix. The weight is first packed (once per weight version) into MFMA fragment order:
 * wpack = ivit_patch_weight_pack_bytes(D, C) bytes, from W [D][C][8][8] f32. D = 384 or 192;
 * img and wpack 16-byte aligned. Same output as ivit_patch_embed_fwd with dtype IVIT_BF16. */
long ivit_patch_weight_pack_bytes(long D, long C);
int ivit_patch_weight_pack(const float* w, long D, long C, void* wpack, void* stream);
int ivit_patch_embed_fwd_packed(const float* img, long B, long C, long H, long W, const void* wpack,
                                const float* bias, const float* pos, const float* cls, long D, float* out,
                                void* stream);

/* ---- Differing patch grids (model_vit.py:64,71 with e.g. vit_small_patch16_224 for one stream,
 *      and the bilinear re-grid of model_vit.py:139).
 * PatchEmbed with patch P != 8 = patch matrix + ivit_linear_fwd + token assembly:
 *   cols[b*Np + gy*Wp + gx][(c*P + ky)*P + kx] = img[b][c][gy*P + ky][gx*P + kx]  (cols_dtype)
 *   out[b][0] = cls + pos[0];  out[b][1 + p] = Y[b*Np + p] + pos[1 + p]           (f32)
 * tokens_bwd: dY[b*Np + p] = dtok[b][1 + p] (dy_dtype, the weight gradient's operand);
 *   dpos (+)= sum_b dtok[b];  dcls (+)= sum_b dtok[b][0].                                    */
int ivit_patch_im2col_p(const float* img, long B, long C, long H, long W, long P, void* cols, int cols_dtype,
                        void* stream);
int ivit_patch_tokens(const float* Y, long B, long Np, long D, const float* pos, const float* cls, float* out,
                      void* stream);
int ivit_patch_tokens_bwd(const void* dtok, int dtok_dtype, long B, long Np, long D, void* dY, int dy_dtype,
                          float* dpos, float* dcls, int accumulate, void* stream);
/* F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False) on Z = B*C planes of
 * Hi x Wi f32 (ATen's linear taps: src = max((o + 0.5) * in/out - 0.5, 0)), and its adjoint
 * dX = R_h^T dY R_w as a gather (deterministic, no atomics; dX is overwritten).             */
int ivit_bilinear_fwd(const float* X, long Z, long Hi, long Wi, float* Y, long Ho, long Wo, void* stream);
int ivit_bilinear_bwd(const float* dY, long Z, long Hi, long Wi, long Ho, long Wo, float* dX, void* stream);

/* ---- Loading pretrained / other-grid checkpoints (timm vision_transformer.checkpoint_filter_fn;
 *      the reference's pretrained_lidar / pretrained_map, model_vit.py:64,71). Load-time only.
 * ivit_pos_resample = timm resample_abs_pos_embed's F.interpolate(mode='bicubic', antialias=True,
 * align_corners=False) of the patch part of pos_embed: src f32 [h, w, D] channels last (the
 * [1, D, h, w] view of pos_embed[0, prefix:], no permute), dst f32 [oh, ow, D]. Separable, width
 * pass then height pass; per axis, n_in -> n_out:
 *   scale = n_in / n_out;  support = scale >= 1 ? 2 scale : 2;  inv = scale >= 1 ? 1 / scale : 1
 *   output i:  c = scale (i + 0.5);  xmin = max(0, (int)(c - support + 0.5));
 *              xmax = min((int)(c + support + 0.5), n_in)
 *   w_j = k((j - c + 0.5) inv) for j in [xmin, xmax), divided by their sum;  out_i = sum_j w_j in_j
 *   k(x) = ((a + 2)|x| - (a + 3)) x^2 + 1        for |x| < 1        (Keys cubic, a = -0.5)
 *        = (((|x| - 5)|x| + 8)|x| - 4) a         for 1 <= |x| < 2;   0 beyond
 * Up-sampling has 4 taps per axis, down-sampling by s about 4 s (any count). Weights, their
 * normalisation and the sums are f64 (the width pass leaves an f64 [h, ow, D] intermediate in
 * work), so the result is the f64 value rounded once to f32; equal sizes reproduce src exactly.
 * A gather, no atomics: bitwise repeatable. work: 8-B aligned, >= ivit_pos_resample_workspace bytes
 * (0 for sizes the op refuses). Refused before any device call: non-positive or > 2^30 sizes, null
 * pointers, a workspace too small.                                                               */
long ivit_pos_resample_workspace(long h, long w, long D, long oh, long ow);
int ivit_pos_resample(const float* src, long h, long w, long D, float* dst, long oh, long ow, void* work,
                      long work_bytes, void* stream);
/* timm adapt_input_conv: conv weight f32 [O, I, kh, kw] -> [O, C, kh, kw].  C == I: copy;
 * I == 3, C == 1: the sum over the input channels;  I == 3, other C: out[:, c] = in[:, c mod 3] *
 * (float)(3.0 / C)  (timm's repeat(1, ceil(C / 3), 1, 1)[:, :C] * (3 / C));  any other I is refused
 * (timm raises NotImplementedError), as are null pointers and non-positive sizes.                 */
int ivit_adapt_input_conv(const float* w_in, long O, long I, long kh, long kw, float* w_out, long C, void* stream);

/* ---- k x k stride-1 "same" convolution on NHWC maps (BasicBlock conv3x3/conv1x1,
 *      model_vit.py:12-17; DetectionHead/IntentionHead conv, heads.py:16,37; k = 5: model_cnn.py:7-9).
 *      Weights packed [Cout][k][k][Cin] (see ivit_pack_conv_weight).                           */
int ivit_conv_fwd(int dtype, const void* X, long B, long H, long W, long Cin, const void* Wp, const float* bias,
                  long Cout, long ks, void* Y, long ldy, int y_dtype, void* stream);
int ivit_conv_dgrad(int dtype, const void* dY, long lddy, long B, long H, long W, long Cout, const void* Wp,
                    long Cin, long ks, void* dX, int dx_dtype, void* stream);
long ivit_conv_wgrad_workspace(long B, long H, long W, long Cin, long Cout, long ks);
int ivit_conv_wgrad(int dtype, const void* dY, long lddy, const void* X, long B, long H, long W, long Cin,
                    long Cout, long ks, float* dWp, float* dbias, int accumulate, void* work, long work_bytes,
                    void* stream);
/* Data gradient on the transposed, tap-flipped pack of ivit_pack_conv_weight_t (bf16; the 288 x 256
 * panel kernel: Cout % 64 == 0, Cin >= 128, Cin % 8 == 0, lddy % 8 == 0, B*H*W >= 288, ks in {1, 3, 5};
 * IVIT_ERR_ARG otherwise); same sums as ivit_conv_dgrad. */
int ivit_conv_dgrad_t(int dtype, const void* dY, long lddy, long B, long H, long W, long Cout, const void* WpT,
                      long Cin, long ks, void* dX, int dx_dtype, void* stream);
/* Convolution + the following BatchNorm2d's training-mode batch statistics in one pass (BasicBlock
 * conv -> bn, model_vit.py:24-27,35-43): Y = conv(X, Wp) (no bias, dense: ldy == Cout) and mean /
 * invstd (biased variance, eps) of Y's channels, running mean / var updated with momentum (unbiased
 * variance) as ivit_bn_stats. bf16 panel shapes fold the statistics into the convolution's epilogue
 * (per-tile sums and centred squares, merged across tiles in a fixed order); other shapes run
 * ivit_conv_fwd + ivit_bn_stats. Either way the statistics are those of Y as stored (of the rounded
 * values for a bf16 Y). */
long ivit_conv_bn_fwd_workspace(long B, long H, long W, long Cout);
int ivit_conv_bn_fwd(int dtype, const void* X, long B, long H, long W, long Cin, const void* Wp, long Cout, long ks,
                     void* Y, long ldy, int y_dtype, float* mean, float* invstd, float* run_mean, float* run_var,
                     float momentum, float eps, void* work, long work_bytes, void* stream);
/* torch [Cout][Cin][k][k] f32  ->  [Cin][k][k][Cout_pad] (dtype) with the taps flipped: the K-contiguous
 * weight of the data gradient, WpT[ci][ky][kx][co] = w[co][ci][k-1-ky][k-1-kx], zero for co >= Cout
 * (the pack for a gradient zero-padded to Cout_pad channels). */
int ivit_pack_conv_weight_t(int dtype, const float* w, long Cout, long Cin, long ks, long Cout_pad, void* out,
                            void* stream);
/* torch [Cout][Cin][k][k] f32  ->  packed [Cout_pad][k][k][Cin] (dtype), rows >= Cout zeroed. */
int ivit_pack_conv_weight(int dtype, const float* w, long Cout, long Cin, long ks, long Cout_pad, void* out,
                          void* stream);
/* packed f32 gradient [Cout_pad][k][k][Cin] -> torch layout [Cout][Cin][k][k] (+= if accumulate). */
int ivit_unpack_conv_grad(const float* gp, long Cout, long Cin, long ks, float* out, int accumulate, void* stream);

/* ---- Multi-head self-attention core: timm Attention -> F.scaled_dot_product_attention
 *      (softmax(Q K^T / sqrt(Dh)) V, no mask, no dropout). qkv: [B, N, 3, H, Dh] rows of 3*H*Dh;
 *      out: [B, N, H*Dh]; lse: [B, H, N] f32 (natural-log-sum-exp of the scaled scores).
 *      IVIT_BF16 is flash-style (no N x N buffer: the workspace holds the backward's row
 *      constants and a prescaled Q copy). IVIT_F32, the exact parity path, materialises the scores:
 *      its workspace is 4 B*H*N*ldS bytes (ldS >= N; twice that for the backward) — 0.49 GB per
 *      sample at N = 4501, H = 6, and 7.8 GB at N = 18 001: sized for the parity tests and
 *      config 1 (B = 1), not for training at scale. Its backward recomputes P as a softmax of
 *      the recomputed scores (rows normalised by their own sum) and does not read lse.       */
long ivit_attn_workspace(int dtype, long B, long N, long H, long Dh, int backward);
int ivit_attn_fwd(int dtype, const void* qkv, long B, long N, long H, long Dh, void* out, float* lse, void* work,
                  long work_bytes, void* stream);
int ivit_attn_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, long B, long N,
                  long H, long Dh, void* dqkv, void* work, long work_bytes, void* stream);
/* bf16 path with the Q block of qkv pre-multiplied by log2(e)/sqrt(Dh) (ivit_linear_fwd_qs):
 * the kernels take exp2 of the raw MFMA output (the running max / -lse as the initial
 * accumulator), no per-score scaling. Same outputs as ivit_attn_fwd / ivit_attn_bwd with dtype
 * IVIT_BF16 on the unscaled q; dqkv is the gradient w.r.t. the UNSCALED q, k, v.            */
int ivit_attn_fwd_q2(const void* qkv, long B, long N, long H, long Dh, void* out, float* lse, void* work,
                     long work_bytes, void* stream);
int ivit_attn_bwd_q2(const void* qkv, const void* out, const void* dout, const float* lse, long B, long N, long H,
                     long Dh, void* dqkv, void* work, long work_bytes, void* stream);
/* The same with the DropPath row skip: skip [B] = the attention branch's per-sample factors. The
 * workgroups of a sample with skip[b] == 0 load nothing and store zeros to their rows of out
 * (forward) or dqkv (backward); that sample's lse and backward row constants stay unwritten (their
 * only readers are the skipped workgroups of the same sample). Other samples: bit-identical.
 * The kept samples' tiles are dealt out evenly over the XCDs (the plain block remap would leave a
 * dropped sample's XCD idle), so the launch gets shorter by about the dropped share.
 * skip == null, or IVIT_KNOB_DROP_SKIP at 0: exactly the plain entry point (which forwards here). */
int ivit_attn_fwd_q2_skip(const void* qkv, long B, long N, long H, long Dh, void* out, float* lse, void* work,
                          long work_bytes, const float* skip, void* stream);
int ivit_attn_bwd_q2_skip(const void* qkv, const void* out, const void* dout, const float* lse, long B, long N,
                          long H, long Dh, void* dqkv, void* work, long work_bytes, const float* skip, void* stream);

/* ---- Windowed attention (ViTDet, Li et al. 2022; no reference counterpart): the same operands as the
 *      global entries above, N = 1 + gh*gw tokens: token 0 is CLS, patch token 1 + r*gw + c sits at
 *      (r, c) of the gh x gw grid. Windows of (wh, ww) patches tile the grid from its top-left corner,
 *      the last row / column of windows smaller when the size does not divide the grid (no padding, no
 *      wrap). A patch query attends to the patch keys of its own window only; CLS is a window of its
 *      own (o_cls = v_cls, its lse its single score). wh * ww <= 256; a window larger than the grid is
 *      the grid. One workgroup per (window, sample, head) holds the window in LDS: no workspace, no
 *      atomics, bitwise repeatable. lse [B, H, N] f32 in the units of the global entry of the same
 *      name (natural log; log2 for _q2). The backward entries read neither out nor lse (rows are
 *      renormalised by their own sum). _q2: bf16 with the Q block prescaled by log2(e)/sqrt(Dh), dqkv
 *      w.r.t. the UNSCALED q, k, v; skip as for ivit_attn_fwd_q2_skip (null: none; zeros for a sample
 *      with factor 0, its lse unwritten; IVIT_KNOB_DROP_SKIP at 0 ignores it). IVIT_ERR_ARG, with
 *      nothing launched, for Dh != 64, wh or ww < 1, wh * ww > 256, N != 1 + gh*gw and
 *      N * B * H > 2^31 - 1 (the launch is one flat grid, at most one workgroup per token and head). */
int ivit_attn_win_fwd(int dtype, const void* qkv, long B, long N, long gh, long gw, long wh, long ww, long H, long Dh,
                      void* out, float* lse, void* stream);
int ivit_attn_win_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, long B, long N,
                      long gh, long gw, long wh, long ww, long H, long Dh, void* dqkv, void* stream);
int ivit_attn_win_fwd_q2(const void* qkv, long B, long N, long gh, long gw, long wh, long ww, long H, long Dh,
                         void* out, float* lse, const float* skip, void* stream);
int ivit_attn_win_bwd_q2(const void* qkv, const void* out, const void* dout, const float* lse, long B, long N, long gh,
                         long gw, long wh, long ww, long H, long Dh, void* dqkv, const float* skip, void* stream);

/* ---- Attention probabilities of chosen query rows (model_vit.py:64,71 -> timm Attention: the rows
 *      softmax(q k^T / sqrt(Dh)) that a forward hook on timm's attention would read; the reference
 *      lists their qualitative analysis as future work). qkv as for ivit_attn_fwd: [B, N, 3, H, Dh]
 *      rows of 3*H*Dh, IVIT_F32 or IVIT_BF16, 16-byte aligned. Request r < R names the query row
 *      (sample[r], token[r]) (device int arrays). out (f32): head_mean = 0 -> [R, H, N],
 *      out[r, h, :] = softmax over all N keys; head_mean = 1 -> [R, N], their mean over the heads,
 *      summed in head order. q_prescaled = 1 (IVIT_BF16 only): the Q block holds q * log2(e)/sqrt(Dh)
 *      as ivit_linear_fwd_qs writes it, and the kernel takes exp2 of the raw dot products. Dot
 *      products and softmax in f32, the row's maximum subtracted, the row normalised by its own sum
 *      (no saved lse: works from an inference-mode forward); no atomics, bitwise repeatable. No
 *      workspace: the scores of the first 15 360 keys wait in LDS (60 KB at most, sized from N by the
 *      launcher), later keys are recomputed, so any N >= 1 runs. A request with sample outside
 *      [0, B) or token outside [0, N) gets a zero row and reads nothing. R = 0 returns 0 without a
 *      launch.                                                                                     */
int ivit_attn_rows(int dtype, const void* qkv, long B, long N, long H, long Dh, int q_prescaled, const int* sample,
                   const int* token, long R, int head_mean, float* out, void* stream);

/* ---- Kernel execution timing (bench.py's roofline figure; no reference counterpart).
 * While armed, ivit_attn_fwd_q2 / ivit_attn_bwd_q2 launch through hipExtLaunchKernel with a
 * start / stop event pair bound to the kernel itself: HIP stamps them at the kernel's own begin
 * and end, not at submission, so kernels of a concurrent stream queued ahead of it do not count
 * (the same interval rocprofv3 --kernel-trace reports). arm(1) clears the records and starts
 * recording, arm(0) stops; read() waits for the recorded events of one tag and returns their
 * launch count and, for the first min(count, cap), each kernel's start / stop in ms relative to
 * the first recorded launch's start (a common origin for all tags, so intervals of kernels on
 * concurrent streams can be merged).                                                          */
enum { IVIT_KT_ATTN_FWD = 0, IVIT_KT_ATTN_BWD_DQ = 1, IVIT_KT_ATTN_BWD_DKV = 2, IVIT_KT_NTAGS = 3 };
int ivit_ktime_arm(int on);
int ivit_ktime_read(int tag, double* start_ms, double* stop_ms, long cap, long* count);

/* ---- Diagnostic per-workgroup stamps (no reference counterpart; tools/panel_stamps.py).
 * buf (device, 8 x u64 per workgroup, cap u64 in all) non-null: the row-panel kernels
 * (ivit_linear_fwd_panel, ivit_linear_dgrad_gelu_panel, ivit_linear_resid_ln_fwd,
 * ivit_linear_dgrad_ln_bwd) launch their stamping builds and write, per workgroup b at
 * buf[8 b ..]: shader clock at entry, at the first K stage's data ready, after the main loop,
 * at exit; 100-MHz real time at entry and exit; HW_ID | XCC_ID << 32; 0. Null: off (default).  */
int ivit_debug_stamps(void* buf, long cap);

/* ---- LayerNorm over the last dim D (timm norm1/norm2/norm eps 1e-6; adapters eps 1e-5).
 *      Input rows r -> (r / rpb) * rstride + roff + r % rpb (rpb = 0: identity) of X (f32).    */
int ivit_layernorm_fwd(const float* X, long ldx, long rpb, long rstride, long roff, long M, long D,
                       const float* gamma, const float* beta, float eps, void* Y, long ldy, int y_dtype,
                       float* mean, float* rstd, void* stream);
/* dX(f32) = dres + LN_bwd(dY);  dXs = dtype(dX * row_scale[m / rows_per_scale]) if non-null;
 * dgamma/dbeta (+)= column sums. work >= ivit_layernorm_bwd_workspace(M, D). dX may alias dres.
 * X, dres and dX use the row map; dY (lddy) and dXs ([M, D] contiguous) use plain rows.      */
long ivit_layernorm_bwd_workspace(long M, long D);
int ivit_layernorm_bwd(const float* X, long ldx, long rpb, long rstride, long roff, long M, long D,
                       const float* gamma, const float* mean, const float* rstd, const void* dY, long lddy,
                       int dy_dtype, const float* dres, float* dX, long lddx, void* dXs, int dxs_dtype,
                       const float* row_scale, long rows_per_scale, float* dgamma, float* dbeta, int accumulate,
                       void* work, long work_bytes, void* stream);

/* ---- BatchNorm2d (train: batch statistics, biased var for normalisation, unbiased for the
 *      running update, momentum 0.1, eps 1e-5) on NHWC [M, C] maps (model_vit.py:24-31). */
long ivit_bn_workspace(long M, long C);
int ivit_bn_stats(const void* X, int x_dtype, long M, long C, float* mean, float* invstd, float* run_mean,
                  float* run_var, float momentum, float eps, void* work, long work_bytes, void* stream);
/* Y = [relu]( (X - mean) * invstd * g + b  [+ R] ), Y/R in y_dtype. */
/* eval-mode statistics of nn.BatchNorm2d (model_vit.py:19-34 in eval): mean = running_mean,
 * invstd = rsqrt(running_var + eps), as torch computes them on the device. */
int ivit_bn_eval_stats(const float* run_mean, const float* run_var, long C, float eps, float* mean, float* invstd,
                       void* stream);
int ivit_bn_apply(const void* X, int x_dtype, long M, long C, const float* mean, const float* invstd,
                  const float* g, const float* b, const void* R, int relu, void* Y, int y_dtype, void* stream);
/* Backward of Y = relu?(BN(X) + R): dYin masked by (Y > 0) if relu; dR = masked dY;
 * dX = invstd*g*(dy - mean(dy) - xhat*mean(dy*xhat)); dg, db (+)= sums. */
int ivit_bn_bwd(const void* X, int x_dtype, const void* Y, int y_dtype, const void* dY, int dy_dtype, long M, long C,
                const float* mean, const float* invstd, const float* g, int relu, void* dX, int dx_dtype, void* dR,
                float* dg, float* db, int accumulate, void* work, long work_bytes, void* stream);

/* ---- Small kernels: casts, column sums, token scatter, AdamW ---------------------------- */
int ivit_cast(const void* x, int x_dtype, void* y, int y_dtype, long n, void* stream);
/* out = (a [+ b]) [* gelu'(pre)] [* row_scale[i / (cols * rows_per_scale)]] elementwise over n values. */
int ivit_add_act_grad(const void* a, int a_dtype, const void* b, int b_dtype, const void* pre, int pre_dtype,
                      const float* row_scale, long row_elems, void* out, int out_dtype, long n, void* stream);
/* Standalone activation modules (nn.GELU exact-erf / nn.ReLU used outside the fused GEMM
 * epilogues, e.g. a caller running adapter_lidar[2] on its own): y = act(x); dx = dy * act'(x). */
int ivit_act_fwd(int act, const void* x, int x_dtype, void* y, int y_dtype, long n, void* stream);
int ivit_act_bwd(int act, const void* dy, int dy_dtype, const void* x, int x_dtype, void* dx, int dx_dtype, long n,
                 void* stream);
int ivit_colsum(const void* X, int x_dtype, long ld, long rpb, long rstride, long roff, long M, long N, float* out,
                int accumulate, void* work, long work_bytes, void* stream);
long ivit_colsum_workspace(long M, long N);
/* Adapter output tokens [B*Np, C] -> slice [.., coff:coff+C] of an NHWC map with ld channels. */
int ivit_copy_cols(const void* src, long lds, void* dst, long ldd, long rows, long cols, int dtype, void* stream);
/* Head output [M, ldh] (det A*7 cols, then intent A*K cols) -> cls [M*A], box [M*A, 6], intent [M*A, K]. */
int ivit_split_heads(const float* h, long ldh, long M, long A, long K, float* cls, float* box, float* intent,
                     void* stream);
int ivit_merge_heads_grad(const float* dcls, const float* dbox, const float* dint, long M, long A, long K,
                          void* dh, long ldh, int dh_dtype, void* stream);
/* torch.optim.AdamW (foreach semantics) over n_tensors tensors given by device pointer tables. */
int ivit_adamw(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
               void* const* exp_avg_sq, const long* sizes, long max_size, float lr, float beta1, float beta2,
               float eps, float weight_decay, float bc1, float bc2_sqrt, void* stream);
/* Same update, and shadows[t] (bf16, may be null per tensor) receives bf16(p_new): the
 * compute-dtype copies the next forward reads (replaces one cast launch per weight per step). */
int ivit_adamw_shadow(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                      void* const* exp_avg_sq, void* const* shadows, const long* sizes, long max_size, float lr,
                      float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                      void* stream);
/* Same update (shadows may be null, or null per tensor) with the non-finite-loss guard of
 * train_vit.py:163-165 / loss.py:190-198 without a host sync: finite (device f32, may be null) = 0
 * skips the whole update. steps_in / steps_out (device f32 [n_tensors], both null or both set,
 * distinct): per-tensor step counts before / after; when set, bc1 / bc2_sqrt are ignored and come
 * from steps_in[t] + 1 in f64 with beta1 / beta2, and a skipped update does not advance the count
 * (torch.optim.AdamW's state['step'] when the reference's disconnected zero loss leaves no grad). */
int ivit_adamw_guarded(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                       void* const* exp_avg_sq, void* const* shadows, const long* sizes, long max_size, float lr,
                       double beta1, double beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                       const float* finite, const float* steps_in, float* steps_out, void* stream);
/* ivit_adamw_guarded's update over a flat chunk list: chunks (device int32 [n_chunks][2]) =
 * (tensor t, chunk c) for every c < ceil(sizes[t] / ivit_adamw_chunk_elems()) of every tensor; one
 * workgroup per chunk (no idle workgroups for the small tensors), 16-B accesses where the arrays
 * allow. shadows may be null or hold null entries. Bit-identical to ivit_adamw_guarded. */
long ivit_adamw_chunk_elems(void);
int ivit_adamw_chunked(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                       void* const* exp_avg_sq, void* const* shadows, const long* sizes, const int* chunks,
                       long n_chunks, float lr, double beta1, double beta2, float eps, float weight_decay, float bc1,
                       float bc2_sqrt, const float* finite, const float* steps_in, float* steps_out, void* stream);
/* ivit_adamw_chunked with a device gradient scale: every gradient element is multiplied by
 * *grad_scale (device f32; null = no multiply, bit-identical to ivit_adamw_chunked) in f32 as it is
 * loaded, before the update; the gradient arrays themselves are not written. With the coef of
 * ivit_grad_norm it is the update torch.nn.utils.clip_grad_norm_ + AdamW make, without the scale pass. */
int ivit_adamw_chunked_scaled(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                              void* const* exp_avg_sq, void* const* shadows, const long* sizes, const int* chunks,
                              long n_chunks, float lr, double beta1, double beta2, float eps, float weight_decay,
                              float bc1, float bc2_sqrt, const float* finite, const float* steps_in,
                              float* steps_out, const float* grad_scale, void* stream);
/* ivit_adamw_chunked_scaled that also moves an exponential moving average of the weights, in the
 * same launch: emas (device table of f32 pointers; null = ivit_adamw_chunked_scaled, bit-identical;
 * a null entry = that tensor is not averaged) and, after the parameter update,
 *   e = e + omd * (p_new - e)   in f32: one subtract, one multiply, one add, never fused
 *   omd = (float)(1.0 - d),  d = ema_warmup ? min(ema_decay, (1 + n) / (10 + n)) : ema_decay   in f64
 * with n = steps_in[t] + 1, the tensor's step count after this update. ema_warmup therefore needs
 * steps_in; a caller that counts on the host passes that step's d as ema_decay with ema_warmup 0.
 * finite = 0 writes nothing, e included. grad_scale null = no gradient multiply. ema_decay must be
 * in [0, 1). */
int ivit_adamw_chunked_ema(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                           void* const* exp_avg_sq, void* const* shadows, const long* sizes, const int* chunks,
                           long n_chunks, float lr, double beta1, double beta2, float eps, float weight_decay,
                           float bc1, float bc2_sqrt, const float* finite, const float* steps_in, float* steps_out,
                           const float* grad_scale, void* const* emas, double ema_decay, int ema_warmup,
                           void* stream);
/* ivit_adamw_chunked_ema with a per-tensor hyper-parameter table, so that parameter groups which
 * differ only in learning-rate scale and weight decay (layer-wise lr decay, no decay on 1-D tensors)
 * share ONE launch: hyper (device f32 [n_tensors][2], 8-B aligned; null = ivit_adamw_chunked_ema,
 * bit-identical) = (lr_scale, weight_decay) of tensor t. Each workgroup reads its tensor's pair once
 * and forms, in f32, before the element loop
 *   lr_t = lr * hyper[t][0]                      one multiply, never fused
 *   keep = fma(-lr_t, hyper[t][1], 1)            p *= keep; ONE rounding, as 1 - lr * wd is formed
 *                                                in the launches above
 *   step = lr_t / bc1                            p -= step * m / (sqrt(v) / bc2_sqrt + eps)
 * so the update of tensor t is, bit for bit, the one ivit_adamw_chunked_ema makes with
 * lr = (float)lr * (float)lr_scale and weight_decay = hyper[t][1], and a host that repeats the three
 * lines on stored values gets the same bits. lr_scale 0 leaves the parameter (and its shadow) as it
 * is while the moments, the count and the average move. The scalar weight_decay is
 * ignored. lr must be finite and >= 0. Everything else (finite, device step counts, f64 bias
 * correction, grad_scale, emas with warmup, shadows) is ivit_adamw_chunked_ema's. */
int ivit_adamw_chunked_pt(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                          void* const* exp_avg_sq, void* const* shadows, const long* sizes, const int* chunks,
                          long n_chunks, float lr, double beta1, double beta2, float eps, float weight_decay,
                          float bc1, float bc2_sqrt, const float* finite, const float* steps_in, float* steps_out,
                          const float* grad_scale, void* const* emas, double ema_decay, int ema_warmup,
                          const float* hyper, void* stream);
/* a[t] <-> b[t] (f32, sizes[t] elements) exchanged in place over the same chunk grid, no third
 * buffer; shadows (may be null or hold null entries) receives bf16 of the new a[t]. Puts the averaged
 * weights into the model and back (optim.ModelEMA.swapped). */
int ivit_swap_chunked(long n_tensors, void* const* a, void* const* b, const long* sizes, const int* chunks,
                      long n_chunks, void* const* shadows, void* stream);

/* ---- Global gradient norm / clipping (torch.nn.utils.clip_grad_norm_, norm_type 2). ---------- */
/* L2 norm over n_tensors f32 tensors given as ivit_adamw_chunked takes them (pointer table, sizes,
 * (tensor, chunk) table). Two launches, no atomics, bitwise repeatable and independent of the
 * tensors' alignment: one workgroup per chunk sums the squares in f64 into workspace
 * (ivit_grad_norm_workspace(n_chunks) bytes, 8-B aligned), one workgroup adds the partials in a
 * fixed order and writes result (device f32 [4]):
 *   result[0] norm   = (float)sqrt(sum)
 *   result[1] coef   = min(1, max_norm / (norm + 1e-6f))   (1 when the norm is not finite)
 *   result[2] finite = (finite_in == null || *finite_in != 0) && isfinite(norm), as 1.0 / 0.0
 *   result[3] 0
 * stats (optional, device f64 [5], zeroed by the caller) accumulates over calls: calls, calls with
 * coef < 1, calls with a non-finite norm, sum and max of the finite norms. n_chunks == 0 writes
 * norm 0, coef 1. max_norm must be > 0. */
long ivit_grad_norm_workspace(long n_chunks);
int ivit_grad_norm(long n_tensors, void* const* grads, const long* sizes, const int* chunks, long n_chunks,
                   float max_norm, const float* finite_in, void* workspace, long workspace_bytes, float* result,
                   double* stats, void* stream);
/* g *= *coef (device f32) in place over the same tensor list and chunk grid; nothing is written
 * when *coef == 1. */
int ivit_grad_scale(long n_tensors, void* const* grads, const long* sizes, const int* chunks, long n_chunks,
                    const float* coef, void* stream);

/* ---- Detection / intention loss (loss.py:58-206): assignment + focal + Smooth-L1 + CE. ----- */
/* gt: [B, Gmax, 5] f32 padded, ngt[B] int32, gint[B, Gmax] int32. keep: [B, NA] f32 0/1 (dominant
 * intent keep mask) or null. stats (f32[8]): focal_sum, box_sum, ce_sum, num_pos, keep_sum, loss,
 * cls_loss, box_loss, intent_loss (written), then [9] the finite flag, [10] max(1, num_pos), [11] the
 * intention term's denominator.
 * Workspace contract (callers may read it after _fwd; _bwd and ivit_det_iou_loss_* do): it starts with
 * the per-anchor targets, at offsets that do not depend on Gmax:
 *   tgt   int32 [B * NA] at byte 0: (cls target + 1) in bits 0-1 (cls -1 = ignored, 0 = negative,
 *         1 = positive), (intent target + 1) << 2 above (intent -1 = none: every non-positive anchor);
 *   box_t f32 [B * NA * 6] at the next 256-byte boundary after tgt, (B * NA * 4 + 255) / 256 * 256: the
 *         six delta targets of the matched GT; only the rows of positive anchors are written.
 * What follows them (per-block partial sums, best anchor per GT) is private to the kernels.         */
long ivit_det_loss_workspace(long B, long NA, long Gmax);
int ivit_det_loss_fwd(const float* cls, const float* box, const float* intent, const float* anchors, long B,
                      long NA, long K, const float* gt, const int* ngt, const int* gint, long Gmax,
                      const float* keep, unsigned dominant_mask, int downsampling, const float* class_w,
                      float pos_thr, float neg_thr, float alpha, float gamma, float beta, float w_cls,
                      float w_box, float w_int, int use_rotated, float* stats, void* work, long work_bytes,
                      void* stream);
int ivit_det_loss_bwd(const float* cls, const float* box, const float* intent, long B, long NA, long K,
                      const float* keep, unsigned dominant_mask, int downsampling, const float* class_w,
                      float alpha, float gamma, float beta, float w_cls, float w_box, float w_int,
                      const float* stats, const float* grad_loss, float* dcls, float* dbox, float* dintent,
                      void* work, long work_bytes, void* stream);

/* ---- Rotated-IoU box regression (no reference code: the reference's box term is Smooth-L1) -- */
/* Element-wise: iou[i] = IoU_rot(boxes[i], targets[i]) (x, y, w, l, yaw rows, f32; computed in f64
 * with the conventions and guards of ivit_rotated_iou) and jac[i][0..4] = dIoU/dboxes[i]. A
 * non-finite coordinate gives NaN. The backward is dboxes[i][k] = grad_iou[i] * jac[i][k].
 * n = 0 is a no-op.                                                                            */
int ivit_riou_pairs_fwd(const float* boxes, const float* targets, long n, float* iou, float* jac, void* stream);
int ivit_riou_pairs_bwd(const float* grad_iou, const float* jac, long n, float* dboxes, void* stream);
/* The opt-in IoU term of the detection loss: box_loss = (sum SmoothL1 + iou_weight * sum_pos
 * (1 - IoU_rot(decode(box, anchor), matched GT))) / max(1, num_pos). _fwd runs right after
 * ivit_det_loss_fwd on the same stream with that call's workspace (det_work, read only: its
 * leading per-anchor targets name the positives) and stats, which it updates: [12] sum(1 - IoU),
 * [13] sum IoU, [14] the normalised term (iou_weight included), [15] the positives' mean IoU,
 * [7] box_loss and [5] loss with the term added; a non-finite new total zeroes [5..8], [14], [15]
 * and the finite flag [9], and a flag that is already 0 stays 0. use_rotated picks the IoU of the
 * matched-GT argmax (the assignment's own); the term's IoU is always the rotated one. _bwd runs
 * right after ivit_det_loss_bwd and adds grad_loss * w_box * iou_weight * (-dIoU/d raw) / max(1,
 * num_pos) into dbox for the positives (nothing when the finite flag is 0).
 * work >= ivit_det_iou_loss_workspace(B, NA) bytes, the same buffer in _fwd and _bwd.           */
long ivit_det_iou_loss_workspace(long B, long NA);
int ivit_det_iou_loss_fwd(const float* box, const float* anchors, long B, long NA, const float* gt, const int* ngt,
                          long Gmax, int use_rotated, float w_box, float iou_weight, const void* det_work,
                          long det_work_bytes, float* stats, void* work, long work_bytes, void* stream);
int ivit_det_iou_loss_bwd(long B, long NA, float w_box, float iou_weight, const float* stats,
                          const float* grad_loss, const void* det_work, long det_work_bytes, const void* work,
                          long work_bytes, float* dbox, void* stream);

/* ---- Geometry (utils.py) -----------------------------------------------------------------
 * ivit_generate_anchors: out [fh*fw*A, 5] with fh = bev_h / stride, fw = bev_w / stride (floor),
 * rows location-major, anchor-minor; bit-equal to the reference's f32 arithmetic. No rows (a side
 * shorter than the stride, A = 0): returns 0 and writes nothing.
 * ivit_axis_iou / ivit_rotated_iou: out [n1, n2] row-major, out[r * n2 + c] = IoU(b1[r], b2[c]) of
 * xywha rows (the axis form reads columns 0..3). Every element of the output is written; n1 = 0 or
 * n2 = 0 returns 0 and writes nothing. Axis: inputs without a NaN follow the reference
 * (compute_axis_aligned_iou in f32, its operation order) bit for bit, zero, negative and infinite
 * sizes included (where that arithmetic gives NaN, so does this); the value for a box with a NaN
 * field is unspecified (fmaxf / fminf drop a NaN that torch.maximum propagates). Rotated: the f64
 * convex clip rounded once to f32, within 2^-24 |iou| + 1e-9 of the exact value for areas >= 0.1
 * and coordinates that f64 resolves to 1e-9 of the box size; an area below 1e-6, an intersection
 * of at most 1e-7 or a union of at most 1e-6 gives exactly 0.
 * ivit_decode_boxes: out[i] = decode(rel[i], anchors[idx ? idx[i] : i]); idx (int64, any order,
 * repeats allowed) gathers from a longer anchor table and gives the bits of the call without it
 * on the gathered rows. The decoded yaw lies in [-pi, pi].                                       */
int ivit_generate_anchors(long bev_h, long bev_w, long stride, const float* cfgs, long A, float voxel, float off_x,
                          float off_y, float* out, void* stream);
int ivit_axis_iou(const float* b1, long n1, const float* b2, long n2, float* out, void* stream);
int ivit_rotated_iou(const float* b1, long n1, const float* b2, long n2, float* out, void* stream);
int ivit_decode_boxes(const float* rel, const float* anchors, const long* idx, long n, float* out, void* stream);
/* torchvision CPU nms semantics, bit-exact: keep (int64, score order), count (int64[1]). */
long ivit_nms_workspace(long n);
int ivit_nms(const float* boxes_xywha, const float* scores, long n, double iou_thr, long* keep, long* count,
             void* work, long work_bytes, void* stream);

/* ---- Detection mAP / intention matching (eval_vit.py:191-292, calculate_ap utils.py:564-575;
 * SURVEY.md §8f rank 2). Sample s: iou rows = its predictions in score order (descending,
 * stable), columns = its GTs: [npred[s], ngt[s]] f32 at iou + iou_off[s]; its predictions occupy
 * pred_off[s] .. pred_off[s] + npred[s] - 1 of the [total_pred] outputs. Per (sample, threshold):
 * ap[s * n_thr + t] (f64) with the reference's empty-set rules; tp[t * total_pred + p] (u8) the
 * greedy TP flags; best_gt[p] (int32) the first-max GT of each prediction (intention pairs are
 * the TPs at 0.5). work >= 8 * n_thr * total_pred bytes; max_gt <= 4096.                     */
int ivit_det_match(const float* iou, const long* iou_off, const int* npred, const int* ngt, const long* pred_off,
                   long n_samples, long total_pred, const float* thresholds, long n_thr, double* ap, int* best_gt,
                   unsigned char* tp, void* work, long work_bytes, int max_gt, void* stream);

/* ---- Detection error breakdown (extends eval_vit.py:191-292: the same matching, then why a
 * prediction or a GT did not count; the reference's "detailed error analysis" future work).
 * iou / iou_off / npred / ngt / pred_off as ivit_det_match; sample s's GTs occupy gt_off[s] ..
 * gt_off[s] + ngt[s] - 1 of gt_boxes / gt_int / gt_status. pred_boxes [total_pred, 5] f32 in score
 * order, gt_boxes [total_gt, 5] f32, both (cx, cy, w, l, yaw) in ego-centric metres; pred_int /
 * gt_int int32 intentions. range_edges: n_edges <= 7 ascending f32 in HOST memory (read before
 * the launch): bin b holds edges[b-1] <= r < edges[b], nb = n_edges + 1 bins. Outputs:
 *   category [total_pred] u8: 0 TP, 1 DUP (best >= thr_fg, not the first of its GT), 2 LOC
 *     (thr_bg <= best < thr_fg), 3 BKG (best < thr_bg, or the sample has no GT);
 *   gt_status [total_gt] u8: 0 MATCHED, 1 MISSED_NEAR (column max >= thr_bg), 2 MISSED_NONE;
 *   best_gt [total_pred] int32 (first-max GT, -1 without GTs);
 *   errors [total_pred, 4] f64: ate, ase, aoe, aoe_pi of a TP against its GT, 0 elsewhere;
 *   tallies [n_samples, nb, 12] f64: counts TP DUP LOC BKG MISSED_NEAR MISSED_NONE GT, sums ate ase
 *     aoe aoe_pi over TPs, TPs whose intention lies outside 0..7 (a TP and a GT are binned by the
 *     GT's centre, every other prediction by its own);
 *   confusion [n_samples, nb, 8, 8] int32 over TPs: GT intention row, predicted intention column;
 *   ap [n_samples, 5] f64: base, no_dup, no_bkg, fix_loc, no_miss (the AP of ivit_det_match over
 *     the variant's kept predictions and GT count; base equals ivit_det_match at thr_fg).
 * Integer LDS atomics and fixed-order f64 sums only: the same input gives the same bits.
 * work >= ivit_det_errors_workspace(n_samples, total_pred) bytes; max_gt <= 4096;
 * 0 <= thr_bg < thr_fg.                                                                        */
long ivit_det_errors_workspace(long n_samples, long total_pred);
int ivit_det_errors(const float* iou, const long* iou_off, const int* npred, const int* ngt, const long* pred_off,
                    const long* gt_off, long n_samples, long total_pred, const float* pred_boxes,
                    const float* gt_boxes, const int* pred_int, const int* gt_int, float thr_fg, float thr_bg,
                    const float* range_edges, int n_edges, unsigned char* category, unsigned char* gt_status,
                    int* best_gt, double* errors, double* tallies, int* confusion, double* ap, void* work,
                    long work_bytes, int max_gt, void* stream);

/* ---- LiDAR BEV voxelisation ----------------------------------------
 * Replaces utils.create_intentnet_lidar_bev (utils.py:62-106) and, when sweep_tf is given, the
 * per-sweep transform_points(pts, rel_tf) of dataset.py:319-340 (utils.py:27-33) in one pass.
 * points: [P, ld] f32 (points_f64 = 0) or f64 rows, x y z in columns 0..2; intensity: [P] f32.
 * Sweep s owns rows sweep_start[s] .. sweep_start[s+1]-1 (int64 prefix offsets, n_sweeps + 1);
 * max_points >= the largest sweep. sweep_tf: [n_sweeps, 4, 4] f64 row-major or null (points
 * already in the current ego frame). Sweep s scatters into planes sweep_plane[s] ..
 * sweep_plane[s] + height_channels - 1 of bev ([planes, H, W] f32), which the caller zero-fills
 * (np.zeros in the reference): bev[c, floor(off_y - x/voxel), floor(off_x + y/voxel)] =
 * max(bev, intensity) for z in [z_min, z_max), c = clip(floor((z - z_min)/z_range * C)).
 * z_range = z_max - z_min as the caller computes it (constants.py). f64 binning, bit-exact. */
int ivit_lidar_bev(const void* points, int points_f64, long ld, const float* intensity, const long* sweep_start,
                   long n_sweeps, long max_points, const double* sweep_tf, const int* sweep_plane, float* bev,
                   long H, long W, long height_channels, double voxel, double off_x, double off_y, double z_min,
                   double z_max, double z_range, void* stream);

/* Batched NMS (eval_vit.py:170 for every sample of a batch, one launch per stage): sample s
 * owns rows seg[s] .. seg[s+1]-1 (int64 device offsets) of boxes / scores / keep and the mask
 * words mask_off[s] .. + n_s * ceil(n_s / 64); keep receives LOCAL kept indices in score order,
 * count[s] their number; the score order is a stable descending radix sort (one workgroup per
 * sample). n_s <= 131072. work >= ivit_nms_batched_workspace(n_samples, total, mask_words) bytes. */
long ivit_nms_batched_workspace(long n_samples, long total, long mask_words);
int ivit_nms_batched(const float* boxes_xywha, const float* scores, const long* seg, const long* mask_off,
                     long n_samples, long total, long max_n, long mask_words, double iou_thr, long* keep,
                     long* count, void* work, long work_bytes, void* stream);

/* Eval post-processing of a batch (replaces the per-sample loop of eval_vit.py:156-176: sigmoid,
 * torch.where(score >= CONFIDENCE_THRESHOLD), decode_box_predictions utils.py:227-257, apply_nms
 * utils.py:259-274, argmax of the intention logits) with no host round trip. cls [B, NA] f32
 * logits, box_rel [B, NA, 6], intent [B, NA, K], anchors [NA, 5]; NA <= 131072. Sample s's kept
 * detections, in NMS (descending score) order, go to rows s*NA .. s*NA + out_count[s] - 1 of
 * out_scores [B, NA], out_boxes [B, NA, 5] (decoded xywha) and out_intent [B, NA] (int64);
 * out_count [B] int64 is the one value the caller reads back. Scores are torch's f32 GPU sigmoid,
 * boxes ivit_decode_boxes', keep order torchvision CPU nms's (bit-exact).
 * work >= ivit_eval_post_workspace(B, NA) bytes: 76 B per row (B * NA rows) for the compacted
 * scores, anchors, boxes, sort scratch, order, corners and keep list, plus the suppression mask,
 * which is reserved for the worst case (every anchor of every sample passes) and dominates:
 * B * NA * ceil(NA / 64) * 8 bytes, about 2.0 GB at B = 32, NA = 22 500.                        */
long ivit_eval_post_workspace(long B, long NA);
int ivit_eval_post(const float* cls, const float* box_rel, const float* intent, const float* anchors, long B, long NA,
                   long K, float conf_thr, double iou_thr, float* out_scores, float* out_boxes, long* out_intent,
                   long* out_count, void* work, long work_bytes, void* stream);

/* Rotated NMS (the reference's future work, "refined evaluation (rotated NMS/IoU)"): the batched
 * NMS and the eval post-processing above with the suppression test on the rotated boxes. Greedy
 * NMS in torchvision's form with the IoU swapped: the order is the same stable descending sort of
 * the scores (ties keep row order, -0 ties with +0); sorted positions are visited in order, an
 * unsuppressed p is kept and suppresses every later q iff (double)rotated_iou(box[p], box[q]) > thr.
 * rotated_iou is ivit_rotated_iou's function (f64 convex clip rounded to f32; area, intersection
 * and union guards give 0) with the higher-ranked box as its FIRST argument (the clip's rounding
 * is not symmetric): the decision for (p, q) equals ivit_rotated_iou(sorted, sorted)[p][q] > thr
 * bit for bit. With thr < 0 every pair suppresses, disjoint ones included. Boxes with NaN / inf
 * fields are decided by that same function, never by the kernel's f32 distance prefilter.
 * Arguments, outputs (kept indices, counts, packed rows) and limits are those of
 * ivit_nms_batched / ivit_eval_post; a single-sample call is n_samples = 1; samples with no rows
 * get count 0. Workspace: the axis-aligned one (the eval form still reserves the worst-case mask,
 * 8 * NA * ceil(NA / 64) bytes per sample) plus 112 bytes per row: 80 for the box's f64 corners
 * and area, 32 for its f32 prefilter record. That is 152 B per row + 8 B per mask word for
 * ivit_nms_rotated_batched and 188 B per row + the mask for ivit_eval_post_rotated.              */
long ivit_nms_rotated_batched_workspace(long n_samples, long total, long mask_words);
int ivit_nms_rotated_batched(const float* boxes_xywha, const float* scores, const long* seg, const long* mask_off,
                             long n_samples, long total, long max_n, long mask_words, double iou_thr, long* keep,
                             long* count, void* work, long work_bytes, void* stream);
long ivit_eval_post_rotated_workspace(long B, long NA);
int ivit_eval_post_rotated(const float* cls, const float* box_rel, const float* intent, const float* anchors, long B,
                           long NA, long K, float conf_thr, double iou_thr, float* out_scores, float* out_boxes,
                           long* out_intent, long* out_count, void* work, long work_bytes, void* stream);

/* Weighted box fusion (box voting) behind the NMS above, and flip test-time augmentation for the
 * eval post-processing. The reference has neither. Candidates of one sample are rows (box xywha
 * f32, score f32, intention int32, view in {0, 1}). The sort, the suppression mask (axis or
 * rotated test) and the greedy walk are those of ivit_nms_batched / ivit_nms_rotated_batched,
 * unchanged; the kept rows are the leaders.
 *   Ownership: a suppressed row q belongs to the first leader p in score order whose mask bit
 *     (p, q) is set, the box that removed it in the walk. Leaders own themselves.
 *   Alignment (f64): d = a_q - a_p, k = the integer nearest d / (pi/2), delta = d - k * pi/2,
 *     (w~, l~) = (l_q, w_q) if k is odd, else (w_q, l_q): (w, l, a) = (l, w, a + pi/2) = (w, l, a + pi).
 *   fuse = 1: with S the sum of the member scores, x = sum(s_q x_q) / S, y, w~, l~ likewise,
 *     a = a_p + sum(s_q delta_q) / S wrapped into (-pi, pi], all in f64 and rounded once to f32
 *     (a fixed summation order: bitwise repeatable, independent of the other samples of the
 *     launch; a cluster whose S is not positive keeps its leader's box); the intention is the
 *     argmax over the K classes of sum(s_q [intention_q = c]), the lowest class on a tie; the
 *     score (f32) is m_0 with one view and (m_0 + m_1) * 0.5f with two, m_v the largest member
 *     score of view v or 0 without one. Fused scores are not thresholded again. Output rows are
 *     in stable descending order of the fused score, ties in leader order.
 *   fuse = 0: box, score and intention are the leader's own, in keep order (plain NMS over the
 *     union of the views).
 * ivit_nms_fuse_batched: segments as ivit_nms_batched (seg, mask_off, max_n, mask_words);
 * intentions [total] int32 in 0..K-1 (K <= 32), views [total] int32 or null (all view 0; ignored
 * with n_views = 1). Sample s's rows go to seg[s] .. seg[s] + count[s] - 1 of out_leader (int64,
 * the leader's LOCAL row), out_boxes [total, 5], out_scores, out_intent (int64) and out_members
 * (int32 cluster sizes, the leader included; may be null).
 * work >= ivit_nms_fuse_batched_workspace(n_samples, total, mask_words, rotated): the NMS
 * workspace plus 28 B per row (keep list, rank, owner and one fused row's score / intention /
 * member count; the fused boxes reuse the sorted-corner rows, dead after the mask).             */
long ivit_nms_fuse_batched_workspace(long n_samples, long total, long mask_words, int rotated);
int ivit_nms_fuse_batched(const float* boxes_xywha, const float* scores, const int* intentions, const int* views,
                          const long* seg, const long* mask_off, long n_samples, long total, long max_n,
                          long mask_words, long K, long n_views, int fuse, int rotated, double iou_thr,
                          long* out_leader, float* out_boxes, float* out_scores, long* out_intent, int* out_members,
                          long* count, void* work, long work_bytes, void* stream);

/* ivit_eval_post over V in {1, 2} views of the same B scenes, view 1 the forward of the mirrored
 * rasters (the training flip: ivit_bev_augment's flip). cls [V, B, NA], box_rel [V, B, NA, 6],
 * intent [V, B, NA, K], one anchor set [NA, 5]. Per sample: sigmoid >= conf_thr per view in anchor
 * order, decode, the row's argmax intention; view 1 un-mirrored (y and the yaw negated, both
 * exactly; the intention through the HOST table flip_intent[K], null = identity); view-0 rows
 * first, then view-1 rows; then the shared sort / mask / walk and the fusion above. Capacity
 * C = V * NA rows per sample, C <= 131072. Outputs as ivit_eval_post with row stride C:
 * out_scores [B, C], out_boxes [B, C, 5], out_intent [B, C] (int64), out_members [B, C] (int32,
 * may be null), out_count [B]; nothing is read back. V = 1, fuse = 0 gives ivit_eval_post's rows
 * bit for bit.
 * work >= ivit_eval_post_tta_workspace(B, V, NA, rotated): ivit_eval_post's layout for B samples
 * of C anchors plus 24 B per row + 4 B per sample. The mask grows with C^2, so a caller that must
 * stay within the workspace it already reserves for ivit_eval_post(B, NA) (rotated:
 * ivit_eval_post_rotated) runs the batch in chunks of Bc samples, Bc the largest value with
 * ivit_eval_post_tta_workspace(Bc, V, NA, rotated) <= ivit_eval_post[_rotated]_workspace(B, NA),
 * at least 1: about B / 4 samples per launch set for two views (utils.tta_chunk).              */
long ivit_eval_post_tta_workspace(long B, long V, long NA, int rotated);
int ivit_eval_post_tta(const float* cls, const float* box_rel, const float* intent, const float* anchors, long V,
                       long B, long NA, long K, const int* flip_intent, float conf_thr, double iou_thr, int rotated,
                       int fuse, float* out_scores, float* out_boxes, long* out_intent, int* out_members,
                       long* out_count, void* work, long work_bytes, void* stream);

/* ---- BEV augmentation passes ----------------------------------------
 * Replaces the raster side of utils.augment_bev (utils.py:500-517): random_flip_bev's np.flip
 * (:399-401), random_rotate_bev's per-channel cv2.warpAffine (:425-438), random_scale_bev's
 * per-channel cv2.resize + centre crop / pad (:455-474) and random_bev_dropout's rectangles
 * (:483-493). passes: device array of n_passes ivit_bev_pass entries (192 B each); entry i reads
 * the [C, H, W] f32 stack at src and writes the one at dst (distinct buffers). All stacks share
 * H x W; max_planes >= every entry's C (C = 0 skips the entry). The caller draws the random
 * parameters (python `random`, the reference's order) and chains passes: flip is fused into
 * the first pass's reads, the dropout rectangles into the last pass's writes.               */
typedef struct ivit_bev_pass {
  unsigned long long src, dst; /* device addresses of plane 0; plane stride H * W floats */
  int C;                       /* planes (0 = skip) */
  int op;                      /* 0 copy, 1 warpAffine INTER_LINEAR / BORDER_CONSTANT 0, 2 resize + crop / pad */
  int flip;                    /* read source columns mirrored (np.flip(axis=2) fused) */
  int n_rect;                  /* dropout rectangles zeroed in the output, 0..5 */
  double m[6];                 /* op 1: the INVERTED 2x3 map dst -> src, as warpAffine inverts M */
  double scale_x, scale_y;     /* op 2: 1 / (new_w / W), 1 / (new_h / H) */
  int new_w, new_h;            /* op 2: resized size (int(W s), int(H s)) */
  int off_x, off_y;            /* op 2: out(y, x) = resized(y + off_y, x + off_x), zero outside */
  int rect[5][4];              /* y0, x0, h, w */
} ivit_bev_pass;
int ivit_bev_augment(const void* passes, long n_passes, long H, long W, long max_planes, void* stream);

/* HD-map rasterisation (utils.py:108-182 rasterize_map_ego_centric):
 * cv2.polylines / cv2.fillPoly (LINE_8, 1 px, shift 0, colour 1) into zero-filled f32 planes.
 * seg [n_seg, 5] int32 (x0, y0, x1, y1, plane bitmask): open-polyline segments AND polygon
 * edges (fillPoly draws every edge with cv::Line); seg_base [n_seg] int64 element offset of the
 * segment's [planes, H, W] image. edges [*, 4] int64 (y0, y1, x_top << 16, dx << 16 truncated)
 * of the non-horizontal polygon edges; polys [n_polys, 3] int32 (first edge, edge count <=
 * max_edges <= 256, plane bitmask), poly_base [n_polys] int64; rows [n_rows, 2] int32
 * (polygon, scanline y) fill work items (polygons with >= 2 edges, y0_min <= y < min(y1_max, H)).
 * Replaces utils.py:148-182's per-lane cv2 calls. */
int ivit_map_raster(const int* seg, long n_seg, const long* seg_base, const long* edges, const int* polys,
                    long n_polys, const long* poly_base, const int* rows, long n_rows, long max_edges, long H, long W,
                    float* out, void* stream);

/* ---- Strided convolutions of the CNN variant (model_cnn.py:7-12, 14-33, 86-100; SURVEY.md
 * §8f rank 4) as im2col + the dense GEMMs above. X: NHWC [B, H, W, C] (f32 or bf16); cols:
 * [B*Ho*Wo, ldc] row (b, oy, ox), column (ky*k + kx)*C + c = X[b, oy*s - pad + ky,
 * ox*s - pad + kx, c] (0 outside the map and in columns k*k*C .. ldc-1), i.e. the
 * [Cout][k][k][Cin] packed weight viewed [Cout, k*k*C] is the GEMM operand; Ho, Wo follow
 * nn.Conv2d (floor((H + 2 pad - k) / s) + 1; H + 2 pad >= k and W + 2 pad >= k). Dtype pairs
 * f32 -> f32, f32 -> bf16 (round to nearest even), bf16 -> bf16. col2im (C <= 512) is the adjoint
 * as a gather: dX (f32, NHWC) = sum over (ky, kx) ascending of the dcols entries whose window
 * covers the pixel (0 where none does); columns k*k*C .. ldc-1 of dcols are not read.       */
int ivit_im2col(int x_dtype, const void* X, long B, long H, long W, long C, long k, long stride, long pad, long Ho,
                long Wo, void* cols, long ldc, int cols_dtype, void* stream);
int ivit_col2im(const float* dcols, long ldc, long B, long H, long W, long C, long k, long stride, long pad, long Ho,
                long Wo, float* dX, void* stream);

/* ---- Heuristic intention labels (heuristic_labeling.py:10-124 get_vehicle_intention_heuristic_enhanced,
 * applied to every row by preprocess_intent_labels.py:41-57) ---------------------------------
 * The reference filters and sorts the whole annotation table once per row; this labels all rows
 * of one or more logs in one launch, one thread per row. Rows are concatenated and sorted by
 * (track, timestamp_ns), unique within a track: ts [n] int64, xy [n, 2] f64 (tx_m, ty_m), quat
 * [n, 4] f64 (qx, qy, qz, qw), is_vehicle [n] u8 (category in VEHICLE_CATEGORIES,
 * preprocess_intent_labels.py:42); track t owns rows track_off[t] .. track_off[t+1]-1 (int64,
 * n_tracks + 1 entries, track_off[0] = 0, track_off[n_tracks] = n). All device pointers; params
 * is a HOST pointer (constants.py values, passed to the kernel by value).
 * intent [n] int32: -1 for a non-vehicle row, else INTENTIONS_MAP (constants.py), OTHER = 7 by
 * default. The future rows (:37) are the min(horizon_steps, rows left in the track) rows after
 * the row; fewer than min_future_points -> OTHER (:38). With the last of them as the end row:
 * dist = |xy_end - xy|, speed = dist / ((double)(ts_end - ts) * 1e-9 + 1e-9) (:40-45); a zero-norm
 * quaternion at either row -> OTHER (:47-52, before the speed test); dh = atan2(sin, cos) of the
 * yaw difference (:50-51); speed < stopped_speed -> PARKED if dist < parked_max_disp else
 * STOPPING_STOPPED (:54-55); speed >= moving_speed: dh > turn_heading TURN_LEFT, dh < -turn_heading
 * TURN_RIGHT (:79-81), keep_heading < |dh| < turn_heading LEFT_/RIGHT_CHANGE_LANE by the sign of
 * dh (:86-88), |dh| <= keep_heading KEEP_LANE if the displacement's component across the current
 * heading is < keep_lane_max_lat (:118-122). f64 throughout, no contraction.
 * yaw [n] f64: the z angle of scipy's extrinsic as_euler('xyz') of the normalised quaternion,
 * atan2(2(wz + xy), 1 - 2(y^2 + z^2)) (exact away from gimbal lock); 0 for a zero norm.
 * MAP CONTEXT IS NOT IMPLEMENTED: this is the reference's map-free branch, what it computes when
 * av2 is not importable (AV2_MAP_AVAILABLE false / static_map None): no intersection test
 * (:61-77, :83-84) and no lane-polygon containment (:93-117). n = 0 succeeds without a launch. */
typedef struct ivit_label_params {
  int horizon_steps;        /* INTENTION_HORIZON_STEPS */
  int min_future_points;    /* 5 (heuristic_labeling.py:16) */
  double stopped_speed;     /* MIN_SPEED_STOPPED */
  double moving_speed;      /* MIN_SPEED_MOVING */
  double turn_heading;      /* HEADING_CHANGE_THRESH_TURN (rad) */
  double keep_heading;      /* HEADING_CHANGE_THRESH_LANE_KEEP (rad) */
  double parked_max_disp;   /* PARKED_MAX_DISP_M */
  double keep_lane_max_lat; /* KEEP_LANE_MAX_LAT_DIST_FALLBACK */
} ivit_label_params;
int ivit_intent_labels(const long* ts, const double* xy, const double* quat, const unsigned char* is_vehicle,
                       const long* track_off, long n, long n_tracks, const ivit_label_params* params, int* intent,
                       double* yaw, void* stream);

/* ---- Masked-autoencoder pre-training (He et al. 2021; mae.py, pretrain_mae.py) -----------------
 * All index arrays are int32 device arrays; nothing here reads device data on the host. D is a
 * multiple of 64; src / dst / fill / add are 16-byte aligned f32.
 *
 * ivit_token_select: dst[b][j][:] = (0 <= idx[b][j] < Ns ? src[b][idx[b][j]][:]
 *                                                        : (fill ? fill[:] : 0)) + (add ? add[j][:] : 0)
 * src [B, Ns, D], idx [B, Nd], fill [D] or null, add [Nd, D] or null, dst [B, Nd, D]. An index outside
 * [0, Ns) means "no source row": src is never read outside its B * Ns rows whatever idx holds. Without
 * `add` the row is a bit copy; with it, one f32 add per element. The one form is (a) the encoder-side
 * gather of CLS + the kept patches, (b) its backward through the inverse index (-1 for a dropped
 * patch: zeros in the same launch, no memset, no atomics), (c) the decoder-side un-shuffle (fill = the
 * mask token, add = the decoder's position table) and (d) the pick of the masked rows for the
 * prediction head, and its backward. The backward forms need idx injective on its in-range entries.
 *
 * ivit_token_fill_grad: dfill[d] (+)= sum over (b, j) with idx[b][j] outside [0, Ns) of dy[b][j][d]:
 * the mask token's gradient. dy [B, Nd, D] f32. Partials per 64-row block, then one fixed-order column
 * pass: no float atomics, bitwise repeatable. accumulate != 0 adds to dfill. work: 4-B aligned,
 * >= ivit_token_fill_grad_workspace bytes (0 for sizes the entry refuses).
 *
 * ivit_mae_loss_fwd / _bwd: mean squared error of the predicted masked patches against the raster.
 * pred [B*Nm, C*P*P] (pred_dtype IVIT_F32 or IVIT_BF16, 16-byte aligned), img [B, C, H, W] f32
 * (16-byte aligned; H and W multiples of P, P = 8 or 16), pidx [B, Nm]: the masked patches' indices
 * into the (H/P) x (W/P) grid, row-major. COLUMN ORDER: column (c*P + ky)*P + kx of pred row
 * (b, m) is compared with img[b][c][gy*P + ky][gx*P + kx], (gy, gx) = divmod(pidx[b][m], W/P): the
 * (c, ky, kx) order of ivit_patch_im2col_p and of patch_embed.proj.weight.reshape(D, -1), NOT the
 * (ky, kx, c) order of the MAE paper's code (its patchify ends in 'nhwpqc'). The target is read out
 * of the raster; no patch matrix exists. With norm_pix != 0 the target of a patch is
 * (t - mean) / sqrt(var + 1e-6), var the unbiased (n - 1) variance over the patch's L = C*P*P values
 * (torch.var); an all-zero patch gives an all-zero target. The forward writes patch_loss [B*Nm] (the
 * mean over L of the squared difference), stats [B*Nm, 2] = (mean, rstd) per patch ((0, 1) without
 * norm_pix), loss [1] (the mean over the B*Nm patches, summed in a fixed order in f64) and finite [1]
 * (f32 1.0 / 0.0: every per-patch loss and the total finite; the flag FusedAdamW.step takes). A pidx
 * entry outside the grid reads nothing, gives that patch a NaN loss and so finite = 0. The backward
 * reads the upstream scalar gout [1] and finite [1] from device memory and writes
 * dpred = gout * 2 (pred - target) / (B*Nm*L) in pred's dtype (16-byte aligned), all zeros when
 * finite is 0. work: 8-B aligned, >= ivit_mae_loss_workspace bytes. */
int ivit_token_select(const float* src, long B, long Ns, long D, const int* idx, long Nd, const float* fill,
                      const float* add, float* dst, void* stream);
long ivit_token_fill_grad_workspace(long B, long Nd, long D);
int ivit_token_fill_grad(const float* dy, long B, long Nd, long D, const int* idx, long Ns, float* dfill,
                         int accumulate, void* work, long work_bytes, void* stream);
long ivit_mae_loss_workspace(long B, long Nm);
int ivit_mae_loss_fwd(const void* pred, int pred_dtype, const float* img, long B, long C, long H, long W, long P,
                      const int* pidx, long Nm, int norm_pix, float* patch_loss, float* stats, float* loss,
                      float* finite, void* work, long work_bytes, void* stream);
int ivit_mae_loss_bwd(const void* pred, int pred_dtype, const float* img, long B, long C, long H, long W, long P,
                      const int* pidx, long Nm, const float* stats, const float* gout, const float* finite,
                      void* dpred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_H */
