/*
 * i2t.h -- C ABI of libi2t_hip.so: the gfx950 (MI355X) kernels under the image-captioning hot path.
 *
 * The reference (iitmdinesh/image2text) is pure Python over torch ops; it has no FFI of its own.  Each entry
 * point below replaces the torch dispatch site cited next to it (paths relative to the reference repo), and is
 * what a reference-side ctypes binding would call (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller (the PyTorch caching allocator);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no hidden allocation, no host sync,
 *     so every call is legal inside hipGraph stream capture;
 *   - return 0 on success, negative I2T_E* otherwise; never throws.  i2t_last_error() gives the message;
 *   - bf16 tensors are raw uint16 bit patterns; "f32" = IEEE float; row-major with an explicit leading dimension
 *     (elements).  bf16 leading dimensions and base pointers must be multiples of 8 elements / 16 bytes;
 *   - all arithmetic accumulates in fp32.
 */
#ifndef I2T_H
#define I2T_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2T_OK 0
#define I2T_EINVAL (-1)   /* bad argument (shape/alignment/unsupported size) */
#define I2T_EHIP (-2)     /* a HIP runtime call failed */

#define I2T_ABI_VERSION 22

int i2t_abi_version(void);
/* copies the last error message of the calling thread into buf (NUL-terminated); returns its length */
int i2t_last_error(char* buf, size_t n);

/* ---------------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue(alpha * op(A)[M,K] . op(B)[K,N])           bf16 MFMA 16x16x32, fp32 accumulate
 *   replaces: every nn.Linear on the path -- layers.py:437-439,452,469 (c_attn/c_proj), :476-485 (MLP),
 *   :537-542 (cross-attn in/out proj), encoder.py:147-149 (projector), vision_encoder_decoder.py:34-37 (bridge),
 *   decoder.py:189,256 (tied lm_head) -- and their autograd backward (dX = dY.W, dW = dY^T.X).
 *   a_kmajor = 0: A stored [M][K] (K contiguous)      a_kmajor = 1: A stored [K][M] (M contiguous)
 *   b_kmajor = 0: B stored [N][K] (K contiguous)      b_kmajor = 1: B stored [K][N] (N contiguous)
 *   epilogue order: v = alpha*acc; v += bias[n]; if aux_out: aux_out[m][n] = bf16(v)  (pre-activation)
 *                   act 1: v = gelu_tanh(v);  act 2: v *= gelu_tanh'(aux_in[m][n])
 *                   dropout (training): drop_mode 1: v = keep(key, m*N+n) ? v*scale : 0  (resid / MLP dropout,
 *                   layers.py:469,485); drop_mode 2: v *= keep(key + n/(N/3), m) ? scale : 0  (the per-token q/k/v
 *                   multipliers of layers.py:454-461 on the fused c_attn output); keep(key, i) = u8(key, i) >= thr, where u8 is
 *                   byte (i & 3) of lowbias32((i >> 2) ^ key) and thr = round(p * 256); scale = 256 / (256 - thr)
 *                   v += residual[m][n] (f32);  accumulate: v += C[m][n] (f32 C only);  store C as f32 or bf16.
 *   K must be a multiple of 8.  Columns [N, ldc) of C are never written.
 * --------------------------------------------------------------------------------------------------------- */
#define I2T_ACT_NONE 0
#define I2T_ACT_GELU 1
#define I2T_ACT_DGELU 2
#define I2T_ACT_GELU_ERF 3  /* exact GELU x Phi(x) (torchvision ViT MLP); generic epilogue class only */
#define I2T_ACT_DGELU_ERF 4 /* v *= gelu_erf'(aux_in[m][n]) */
#define I2T_ACT_GELU_DOUT 5 /* C = gelu_tanh(v) and aux_out = gelu_tanh'(v) (bf16) instead of the pre-activation: the layer's backward is then */
#define I2T_ACT_MUL_AUX 6   /* v *= aux_in[m][n] -- one multiply per element where I2T_ACT_DGELU re-evaluates exp + rcp (the GELU' epilogue */
                            /* of a K = 512 GEMM cost ~8 us of VALU per 256 x 256 tile against 11.6 us of MFMA work) */
int i2t_gemm_bf16(void* stream,
                  const void* A, int lda, int a_kmajor,
                  const void* B, int ldb, int b_kmajor,
                  void* C, int ldc, int c_is_f32,
                  int M, int N, int K, float alpha,
                  const float* bias, int act,
                  const void* aux_in, int ld_aux_in,
                  void* aux_out, int ld_aux_out,
                  const float* residual, int ldr,
                  int accumulate,
                  int drop_mode, unsigned drop_key, unsigned drop_thr, float drop_scale);
/* The same call with a gradient normaliser folded in: alpha_sumsq (device scalar, or NULL) = sum(g^2) of the tensor the A operand was
 * cut from; alpha is then multiplied by 1 / (sqrt(*alpha_sumsq) + 1e-6) on the device (reference models/functions.py:19-24 divides the
 * block-output gradient by its norm + 1e-6: the backward GEMMs of the block's last linear read the UN-normalised bf16 gradient and
 * apply the factor in their epilogues, so no pass over the gradient exists just to rescale it). */
int i2t_gemm_bf16_ex(void* stream,
                  const void* A, int lda, int a_kmajor,
                  const void* B, int ldb, int b_kmajor,
                  void* C, int ldc, int c_is_f32,
                  int M, int N, int K, float alpha,
                  const float* bias, int act,
                  const void* aux_in, int ld_aux_in,
                  void* aux_out, int ld_aux_out,
                  const float* residual, int ldr,
                  int accumulate,
                  int drop_mode, unsigned drop_key, unsigned drop_thr, float drop_scale,
                     const float* alpha_sumsq);

/* Fused cross-attention forward (reference models/layers.py:537-542,600-605: nn.MultiheadAttention over the encoder output):
 *   kv[b][key][0:d | d:2d] = mem[b][key][:] . [W_k ; W_v]^T + bias_kv          (bf16, written once: the backward pass reads it)
 *   o[q][64 h ..] = softmax(Q_h K_h^T / 8) V_h   per image b and head h,  lse as i2t_attention_fwd
 * in ONE launch: the K/V projection is the persistent 256 x 256 MFMA GEMM, tiled so that a wave ends its K loop holding K_h(b)^T and
 * V_h(b) of one (image, head) in its accumulators, and that wave runs the image's attention straight out of those registers
 * (csrc/gemm.hip::xattn_epilogue) -- K and V are never read back from HBM in the forward.
 * S (memory tokens per image) is 64, or 8 / 16 / 32: a wave's 64 memory rows are then 64 / S whole images, each attended with its own
 * query rows over the key blocks it owns (csrc/gemm.hip::xattn_small_epilogue, epilogue class 16; B S need not fill a tile).  Any
 * other S is refused.
 * mem bf16 [B*S][ld_mem], w_kv = in_proj_weight rows d..3d (bf16 [2d][ld_w], d = 64 H, H even), bias_kv f32 [2d];
 * q / o bf16: [B][Tq] views (batch / row strides) or, with cu_q (device int[B+1]), packed rows (batch strides unused, Tq = max);
 * dropout on the probabilities: same index space and rule as i2t_attention_fwd with Tk = S (drop_thr 0 = off; B H Tq S < 2^32), so i2t_attention_bwd on the
 * stored q / kv / o / lse is its backward. */
int i2t_xattn_kv_fused(void* stream, const void* mem, int ld_mem, const void* w_kv, int ld_w, const float* bias_kv,
                       const void* q, long q_bs, int q_rs, const int* cu_q, int total_q, void* kv, int ld_kv, void* o,
                       long o_bs, int o_rs, float* lse, int B, int S, int H, int Tq, unsigned drop_key, unsigned drop_thr,
                       float drop_scale);

/* column sums: out[n] (+)= sum_m X[m][n]  (bias gradients; X bf16 [M][ld]) */
/* i2t_gemm_bf16 for row-major operands with few output tiles and a long K (a decode step at a mid-sized caption batch): K is cut
 * into slices, each (tile, slice) workgroup writes its raw accumulators to its own [M][N] fp32 plane of `workspace` (ws_floats
 * floats), a second launch adds the planes in slice order and applies the epilogue -- bias, act NONE | GELU, fp32 residual, bf16 or
 * fp32 C.  Deterministic (no atomics).  Falls through to i2t_gemm_bf16 when splitting does not pay, M <= 64 (the weight-streaming
 * kernel), M > 2048 (the planes' traffic outweighs the idle CUs) or the workspace is too small. */
int i2t_gemm_bf16_ws(void* stream, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int c_is_f32, int M, int N, int K,
                     const float* bias, int act, const float* residual, int ldr, float* workspace, long ws_floats);

/* The large-tile GEMM kernels are persistent: one 8-wave workgroup per CU holds the CU's whole LDS and register file and
 * walks a static share of the output tiles.  A kernel from another stream that needs whole CUs for a long time (an RCCL
 * collective overlapped with the backward pass) would leave that many GEMM workgroups waiting for a second round, i.e. double
 * the GEMM's duration.  i2t_gemm_reserve_cus(n) makes later launches leave n CUs free (0 = use every CU again); the
 * data-parallel gradient exchange brackets its overlap window with it (training/dp.py).  Process-wide, takes effect at the
 * next launch. */
int i2t_gemm_reserve_cus(int n_reserved);
/* the reservation currently in force (>= 0); never fails */
int i2t_gemm_reserved_cus(void);

int i2t_colsum_bf16(void* stream, const void* X, int ld, int M, int N, float* out, int accumulate);
/* out[n] (+)= (sum_m X[m][n]) / (sqrt(*alpha_sumsq) + 1e-6)  (alpha_sumsq NULL: plain sums): the bias gradient of a linear layer whose
 * output gradient X is kept un-normalised (see i2t_gemm_bf16_ex) */
int i2t_colsum_bf16_ex(void* stream, const void* X, int ld, int M, int N, float* out, int accumulate, const float* alpha_sumsq);
/* A weight gradient and its bias gradient from one read of dY:
 *   C[M][N] += alpha f A^T . B        colsum_out[m] += f sum_k A[k][m]        f = 1 / (sqrt(*alpha_sumsq) + 1e-6), or 1 when alpha_sumsq is NULL
 * A = dY bf16 [K][lda], B = x bf16 [K][ldb] (both k-major: M is the layer's N, N the layer's K, K the rows), C f32.  The same call as
 * i2t_gemm_bf16_ex(a_kmajor = b_kmajor = accumulate = 1) followed by i2t_colsum_bf16_ex(accumulate = 1) on A; where the GEMM runs as K
 * slices on the persistent kernel the sums are a by-product of that launch (the A fragments a wave holds, once more against an all-ones
 * operand) and A is not read a second time.  Every other route, deterministic mode and I2T_FOLD_COLSUM=0 launch the column-sum kernel.
 * colsum_out NULL: the GEMM alone. */
int i2t_gemm_dw_colsum_bf16(void* stream, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                            float alpha, const float* alpha_sumsq, float* colsum_out);

/* ---------------------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (layers.py:349-358, F.layer_norm eps 1e-5, optional bias)
 *   fwd: x f32 [M][d] -> y (bf16 or f32) [M][d]; saves mean/rstd f32 [M] when non-null
 *   bwd: dx[M][d] (f32) (+)= LN'(dy); dgamma/dbeta f32 [d] are ACCUMULATED (atomics); dy bf16 or f32;
 *        dx_bf16 (nullable): bf16 copy of the final dx rows, i.e. the A operand of the next backward GEMMs
 * --------------------------------------------------------------------------------------------------------- */
int i2t_layernorm_fwd(void* stream, const float* x, const float* gamma, const float* beta,
                      void* y, int y_is_f32, float* mean, float* rstd, int M, int d);
/* the same forward with an explicit eps (torchvision's ViT blocks: 1e-6); the backward only needs the saved rstd */
int i2t_layernorm_fwd_eps(void* stream, const float* x, const float* gamma, const float* beta,
                          void* y, int y_is_f32, float* mean, float* rstd, int M, int d, float eps);
int i2t_layernorm_bwd(void* stream, const void* dy, int dy_is_f32, const float* x, const float* gamma,
                      const float* mean, const float* rstd,
                      float* dx, int dx_accumulate, void* dx_bf16, float* dgamma, float* dbeta, int M, int d,
                      unsigned drop_key, unsigned drop_thr, float drop_scale, float* sumsq_out, const float* dx_pre_sumsq);
/* dx_mask_* (nullable by thr = 0): an elementwise dropout mask (index row * d + column, i2t_dropout_apply mode 1) applied to the f32 dx
 * this call stores -- the embedding dropout's backward (decoder.py:243, encoder.py:170) folded into the lowest block's last LayerNorm
 * backward; sumsq_out and the bf16 copy see the unmasked value */
int i2t_layernorm_bwd_ex(void* stream, const void* dy, int dy_is_f32, const float* x, const float* gamma,
                         const float* mean, const float* rstd,
                         float* dx, int dx_accumulate, void* dx_bf16, float* dgamma, float* dbeta, int M, int d,
                         unsigned drop_key, unsigned drop_thr, float drop_scale, float* sumsq_out, const float* dx_pre_sumsq,
                         unsigned dx_mask_key, unsigned dx_mask_thr, float dx_mask_scale, int acc_period, int acc_rows);
/* acc_period / acc_rows (0 = every row): with dx_accumulate, only rows r with r % acc_period < acc_rows are added onto -- the others
 * are written.  The encoder's CLS-only last block (encoder.py:172-173): dx holds the CLS rows' residual gradient and nothing else, so
 * the zero fill of the patch rows and its read-back are not needed. */
/* dx_pre_sumsq (bwd, nullable, needs dx_accumulate): the dx accumulated onto is still un-normalised -- its old value is
 * multiplied by 1 / (sqrt(*dx_pre_sumsq) + 1e-6) while adding (the gradient normaliser of i2t_grad_normalize flag 2).
 * sumsq_out (bwd, nullable): += sum of squares of the f32 dx written by this call (after accumulation) -- lets the
 * gradient normaliser that consumes dx next skip its own reduction pass (i2t_grad_normalize presummed).
 * drop_* (bwd): optional elementwise dropout (rule of i2t_gemm_bf16, idx = row*d + col, drop_thr 0 = off) applied to the
 * bf16 copy dx_bf16 only -- the copy feeds the backward of a dropped-out branch, the f32 dx is the residual gradient. */

/* ---------------------------------------------------------------------------------------------------------
 * LayerNormND (layers.py:361-370 via encoder.py:150,166,170): one normalisation per image over the joint
 *   (rows x d) slab, affine (rows, d).   y[b] = LN(x[b] + add) * gamma + beta   (add = wpe or NULL)
 *   x,add,gamma,beta f32; y f32 with its own batch stride (lets the 2nd call write behind the CLS rows);
 *   stats = workspace f32 [B][I2T_LNND_STATS_STRIDE]: (mean, rstd) then per-split partials; written by fwd,
 *   read (and its partial slots reused) by bwd.  Each LayerNormND application needs its own stats buffer.
 *   bwd: dx[b] (f32, own batch stride, overwritten) ; dgamma/dbeta (+ dadd when non-null) accumulated.
 * --------------------------------------------------------------------------------------------------------- */
#define I2T_LNND_STATS_STRIDE 34
int i2t_layernorm_nd_fwd(void* stream, const float* x, const float* add, const float* gamma, const float* beta,
                         float* y, long y_batch_stride, float* stats, int B, int rows, int d);
/* the same with the elementwise dropout of the tensor that y is a slab of (the embedding dropout of encoder.py:170 applied by the producer of
 * the patch rows): element (b, i) of y is dropped by the decision of index b * y_batch_stride + drop_base + i (i2t_dropout_apply mode 1's rule) */
int i2t_layernorm_nd_fwd_drop(void* stream, const float* x, const float* add, const float* gamma, const float* beta,
                              float* y, long y_batch_stride, float* stats, int B, int rows, int d,
                              unsigned drop_key, unsigned drop_thr, float drop_scale, long drop_base);
int i2t_layernorm_nd_bwd(void* stream, const float* dy, long dy_batch_stride, const float* x, const float* add,
                         const float* gamma, const float* stats, float* dx, float* dgamma, float* dbeta,
                         float* dadd, int B, int rows, int d);

/* ---------------------------------------------------------------------------------------------------------
 * Attention, head_dim 64 (F.scaled_dot_product_attention at layers.py:465 and inside nn.MultiheadAttention
 *   layers.py:537-542).  softmax(q k^T / 8 [+ causal]) v per (batch, head).
 *   q/k/v/o are bf16 with element strides: batch stride, row (token) stride; head h starts at column 64*h.
 *   Packed c_attn output: q=base, k=base+d, v=base+2d, row stride 3d.  lse f32 [B][H][Tq] (natural log).
 *   causal: key j visible to query i iff j <= i + (Tk - Tq)   (Tk == Tq in training; Tk > Tq with a KV cache)
 *   bwd: dq/dk/dv written (not accumulated), same strides convention as their forward operands.
 *   packed variable-length batches (training skips the caption rows past the last label: they are dead under the causal
 *   mask and carry zero loss weight): cu_q / cu_k (device int[B+1], nullable) give sequence b the rows [cu[b], cu[b+1]) of
 *   a packed [total, width] tensor (batch strides then unused; Tq/Tk = the maxima); with cu_q, lse/delta are [H][total_q].
 *   dropout on the attention probabilities (SDPA dropout_p, layers.py:465; nn.MultiheadAttention dropout): drop_thr = round(p*256)
 *   (0 = off), probability (b,h,q,key) kept iff u8(drop_key, ((b*H+h)*Tq+q)*Tk+key) >= drop_thr, scaled by drop_scale.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_attention_fwd(void* stream, const void* q, long q_bs, int q_rs, const void* k, long k_bs, int k_rs,
                      const void* v, long v_bs, int v_rs, void* o, long o_bs, int o_rs, float* lse,
                      int B, int H, int Tq, int Tk, int causal, unsigned drop_key, unsigned drop_thr, float drop_scale,
                      const int* cu_q, const int* cu_k, int total_q);
int i2t_attention_bwd(void* stream, const void* q, long q_bs, int q_rs, const void* k, long k_bs, int k_rs,
                      const void* v, long v_bs, int v_rs, const void* o, long o_bs, int o_rs,
                      const void* d_o, long do_bs, int do_rs, const float* lse, float* delta_ws,
                      void* dq, long dq_bs, int dq_rs, void* dk, long dk_bs, int dk_rs,
                      void* dv, long dv_bs, int dv_rs, int B, int H, int Tq, int Tk, int causal,
                      unsigned drop_key, unsigned drop_thr, float drop_scale,
                      const int* cu_q, const int* cu_k, int total_q,
                      unsigned out_drop_key, unsigned out_drop_thr, float out_drop_scale);
/* out_drop_* (bwd): the per-token q/k/v multipliers of the fused c_attn output (i2t_gemm_bf16 drop_mode 2) applied to
 * dq / dk / dv on the way out: row r of dq is scaled by keep(key, r), of dk by keep(key + 1, r), of dv by keep(key + 2, r);
 * r = token index (b*T + t, or the packed row).  out_drop_thr 0 = off. */
/* the same with out_drop_q_seq != 0: the Tq query rows are the FIRST rows of sequences of out_drop_q_seq rows (the encoder's last
 * block computes its CLS rows only, layers.py:465 over encoder.py:172-173's slice), so row r of dq is token b*out_drop_q_seq + t in the
 * index space of the multipliers; 0 = Tq.  Offered by the dense resident-operand kernel only. */
int i2t_attention_bwd_ex(void* stream, const void* q, long q_bs, int q_rs, const void* k, long k_bs, int k_rs,
                         const void* v, long v_bs, int v_rs, const void* o, long o_bs, int o_rs,
                         const void* d_o, long do_bs, int do_rs, const float* lse, float* delta_ws,
                         void* dq, long dq_bs, int dq_rs, void* dk, long dk_bs, int dk_rs,
                         void* dv, long dv_bs, int dv_rs, int B, int H, int Tq, int Tk, int causal,
                         unsigned drop_key, unsigned drop_thr, float drop_scale,
                         const int* cu_q, const int* cu_k, int total_q,
                         unsigned out_drop_key, unsigned out_drop_thr, float out_drop_scale, int out_drop_q_seq);

/* ---------------------------------------------------------------------------------------------------------
 * Token + position embedding (decoder.py:231-243): x[b][t] = wte[ids[b][t]] + wpe[t + pos_offset]  (f32)
 *   bwd: dwte[ids] += dx (atomics), dwpe[t+pos_offset] += sum_b dx[b][t]
 *   pos (device int[B*T], nullable): explicit position of every row for packed variable-length batches (then B*T is just
 *   the row count and the wpe gradient is accumulated with atomics).
 *   ids outside [0, vocab) are CLAMPED, forward and backward: id < 0 reads / adds into row 0, id >= vocab row vocab - 1 (no table row
 *   past the vocabulary is ever touched).  wpe NULL (fwd): the token rows alone; dwte / dwpe NULL (bwd): that gradient is skipped.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_embed_fwd(void* stream, const int64_t* ids, const float* wte, const float* wpe, float* x,
                  int B, int T, int d, int pos_offset, int vocab, const int* pos);
int i2t_embed_bwd(void* stream, const int64_t* ids, const float* dx, float* dwte, float* dwpe,
                  int B, int T, int d, int pos_offset, int vocab, const int* pos);

/* ---------------------------------------------------------------------------------------------------------
 * Weighted cross-entropy over bf16 logits (wrapper.py:147-151: F.cross_entropy(logits/T, labels, ignore_index,
 *   'none') * weights, summed).  logits [M][ld] bf16, V valid columns; labels int64 [M] (ignore_index rows skip);
 *   fwd: lse[m] = logsumexp(logits[m]/T); loss += sum_m w[m]*(lse[m] - logits[m][label]/T)   (atomic into *loss)
 *   bwd: logits[m][:] <- bf16( gscale * w[m]/T * (softmax(logits[m]/T) - onehot) ), in place;  gscale read
 *        from device memory (*gscale_ptr) so the upstream gradient never needs a host sync.
 *   DEAD rows: a row whose label is ignore_index, or any other label < 0 or >= V, is dead in every form below: lse[m] = 0, no loss
 *   term, and its V gradient columns are written as zeros.  The pad columns [V, ld) are never written.
 *   The logits must be FINITE: the streaming forms keep a running (max, sum) that starts at -inf, so a leading -inf logit makes
 *   online_add evaluate exp(-inf - -inf) = NaN; +inf and NaN poison the row in every form.  The host does not scan them.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_ce_fwd(void* stream, const void* logits, int ld, const int64_t* labels, const float* w, float inv_temp,
               int64_t ignore_index, float* lse, float* loss, int M, int V);
int i2t_ce_bwd(void* stream, void* logits, int ld, const int64_t* labels, const float* w, float inv_temp,
               int64_t ignore_index, const float* lse, const float* gscale_ptr, int M, int V);
/* One-pass form for training steps (V <= 65536): reads every live row ONCE, leaves lse[m] and the loss term as i2t_ce_fwd does and
 * overwrites the row with the UN-scaled gradient bf16(w[m]/T (softmax(z/T) - onehot)) (dead rows: zeros).  The upstream gradient is
 * applied afterwards with i2t_scale_bf16 (x[0..n) *= *scale_ptr in place; returns without touching x when the scale is exactly 1). */
int i2t_ce_fwd_bwd(void* stream, void* logits, int ld, const int64_t* labels, const float* w, float inv_temp,
                   int64_t ignore_index, float* lse, float* loss, int M, int V);
int i2t_scale_bf16(void* stream, void* x, long n, const float* scale_ptr);
/* Momentum-distillation loss (reference training/wrapper.py:134-144): targets alpha * softmax(teacher/T) + (1 - alpha) * onehot.
 * teacher = the momentum twin's logits of the same rows (bf16 [M][ld_t], constant); lse_t [M] keeps its row lse for backward.
 *   fwd: loss += sum_m w[m] (lse[m] - (1 - alpha) z[m][label]/T - alpha/T sum_v softmax(teacher[m]/T)[v] z[m][v])
 *   bwd: z[m][:] <- bf16(gscale w[m]/T (softmax(z[m]/T) - (1 - alpha) onehot - alpha softmax(teacher[m]/T))), in place. */
int i2t_ce_distill_fwd(void* stream, const void* logits, int ld, const void* teacher, int ld_t, float alpha, const int64_t* labels,
                       const float* w, float inv_temp, int64_t ignore_index, float* lse, float* lse_t, float* loss, int M, int V);
int i2t_ce_distill_bwd(void* stream, void* logits, int ld, const void* teacher, int ld_t, float alpha, const int64_t* labels,
                       const float* w, float inv_temp, int64_t ignore_index, const float* lse, const float* lse_t,
                       const float* gscale_ptr, int M, int V);
/* EMA update of the momentum twin's flat arena (wrapper.py:52-59): pm <- pm momentum + p (1 - momentum); pm_bf16 (nullable) = its shadow */
int i2t_ema_update(void* stream, float* pm, const float* p, void* pm_bf16, long n, float momentum);
/* Decoder inputs of a training step from its labels (wrapper.py:154-196): ids[b][0] = bos, ids[b][t] = label t-1 (ignored -> eos), with
 * the optional MLM corruption of labelled tokens: with probability mask_fraction -> mask_id, or (random_fraction of those) a random
 * id in [0, vocab); draws are counter hashes of (seed, element) -- image2text_amd/rng.py::mlm_draws is the host replica. */
int i2t_lm_inputs(void* stream, const int64_t* labels, int64_t* ids, int B, int L, int64_t bos, int64_t eos, int64_t mask_id, int vocab,
                  int64_t ignore_index, float mask_fraction, float random_fraction, unsigned seed_lo, unsigned seed_hi);


/* ---------------------------------------------------------------------------------------------------------
 * Gradient normaliser (functions.py:19-24): g <- g / (||g||_2 + 1e-6) over the whole f32 tensor, in place.
 *   ws = 1 float of zero-initialised-by-the-call scratch; g_bf16 (nullable) receives a bf16 copy of the result.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_grad_normalize(void* stream, float* g, long n, float* ws, void* g_bf16,
                       unsigned drop_key, unsigned drop_thr, float drop_scale,      /* dropout on the bf16 copy, as i2t_layernorm_bwd */
                       int presummed, float* clear_after);
/* ws[0] (+)= sum(g^2): the first half of i2t_grad_normalize on its own.  Two gradient tensors that the reference normalises as ONE
 * (the prompt rows and the text rows of the decoder when a loss differentiates both) sum their parts and normalise with
 * i2t_grad_normalize(..., presummed = 1). */
int i2t_sumsq(void* stream, const float* g, long n, float* ws, int accumulate);
/* presummed bit 0: *ws already holds sum(g^2) (accumulated by the producer through i2t_layernorm_bwd's sumsq_out) and the
 * reduction pass is skipped; bit 1 (2): g itself is left as it is and only the normalised bf16 copy is written -- the first
 * i2t_layernorm_bwd that accumulates onto g applies the factor (its dx_pre_sumsq = ws), 6 instead of 10 bytes per element;
 * clear_after (nullable): a float zeroed after the call, i.e. the accumulator of the next producer. */

/* ---------------------------------------------------------------------------------------------------------
 * ConvMLP feature extractor (layers.py:258-282): Conv2d(k x k, padding='same', k even => pad (k-1)/2 before,
 *   k/2 after), GELU(tanh) applied to the INPUT when in_gelu (the previous layer stores pre-activations).
 *   x: in_is_f32 ? f32 : bf16 [B][Cin][H][W];  w f32 [Cout][Cin][k][k];  y bf16 [B][Cout][H][W] (pre-activation)
 *   bwd_data:  dx[B][Cin][H][W] bf16 = convT(dy) * (in_gelu ? gelu'(x) : 1)     (skipped for the first layer)
 *   bwd_weight: dw f32 [Cout][Cin][k][k], db f32 [Cout] accumulated (atomics)
 *   w_ws: f32 scratch of Cout*Cin*k*k elements (weights repacked tap-major for scalar loads)
 * --------------------------------------------------------------------------------------------------------- */
int i2t_conv_fwd(void* stream, const void* x, int in_is_f32, int in_gelu, const float* w, const float* bias,
                 void* y, float* w_ws, int B, int Cin, int Cout, int H, int W, int k);
int i2t_conv_bwd_data(void* stream, const void* dy, const float* w, const void* x, int in_gelu, void* dx,
                      float* w_ws, int B, int Cin, int Cout, int H, int W, int k);
int i2t_conv_bwd_weight(void* stream, const void* dy, const void* x, int in_is_f32, int in_gelu,
                        float* dw, float* db, int B, int Cin, int Cout, int H, int W, int k);

/* MFMA implicit-GEMM form of the same 6x6 convolutions (the path the engine uses when every intermediate channel
 * count is 8, 16 or 32).  Layout codes: 0 = NCHW f32 (the image), 1 = NCHW bf16, 2 = NHWC bf16.  Intermediate
 * pre-activations are NHWC bf16; the last layer writes NCHW bf16 (y_nchw) because its output is the flat-patch operand
 * of the projector GEMM (encoder.py:166), whose gradient therefore arrives NCHW (dy_layout 1).
 *   w_ws:    >= 32*36*32 bf16 scratch (weights repacked [co][tap][ci], flipped + transposed for bwd_data)
 *   scratch: >= 32*36*16 f32 (partial dW in [co][tap][ci] order, folded into dw[Cout][Cin][6][6] by the call)
 *   bwd_data: dx (NHWC bf16, Cin channels) = convT(dy) * gelu'(x_pre);  bwd_weight: dw, db accumulated. */
int i2t_conv6_fwd(void* stream, const void* x, int x_layout, int in_gelu, const float* w, const float* bias,
                  void* y, int y_nchw, void* w_ws, int B, int Cin, int Cout, int H, int W);
int i2t_conv6_bwd_data(void* stream, const void* dy, int dy_layout, const float* w, const void* x_pre, void* dx,
                       void* w_ws, int B, int Cin, int Cout, int H, int W);
int i2t_conv6_bwd_weight(void* stream, const void* dy, int dy_layout, const void* x, int x_layout, int in_gelu,
                         float* dw, float* db, float* scratch, int B, int Cin, int Cout, int H, int W);
/* dst[b][y][x][c] = src[b][c][y][x] (bf16, C <= 32): the flat-patch gradient of the last conv layer -> channels-last */
int i2t_nchw_to_nhwc_bf16(void* stream, const void* src, void* dst, int B, int C, int H, int W);

/* ---------------------------------------------------------------------------------------------------------
 * Elementwise / arena utilities
 *   cast:  dst bf16[n] = src f32[n]                     (bf16 weight shadows after an optimizer step)
 *   adamw: torch.optim.AdamW semantics (decoupled decay, bias correction from `step`), one launch over a flat
 *          f32 arena; also refreshes the bf16 shadow of every parameter.  lr/wd are per-element-range tables:
 *          seg_end[i] = exclusive end of segment i, seg_lr[i], seg_wd[i] (nseg small; device arrays).  A segment with
 *          seg_lr < 0 is FROZEN (requires_grad off, or in no parameter group): skipped entirely -- no state, no update, no traffic.
 *          Every seg_end must be a MULTIPLE OF 4 (the arena aligns parameters to 8): a thread updates one float4 with the lr / wd
 *          of the segment its first element lies in.  seg_lr == 0: p and its shadow keep their value (the decay factor is 1), the
 *          moments advance.  p_bf16 NULL: no shadow.  The bias corrections 1 - beta^step are fp32 powf on the host (step >= 1).
 *   add_rows / cls concat helpers for the encoder token buffer.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_cast_f32_bf16(void* stream, const float* src, void* dst, long n);
/* hi[i] = bf16(f(src[i])), lo[i] = bf16(f(src[i]) - hi[i]) (lo may be null); f by act: I2T_ACT_NONE, I2T_ACT_GELU, I2T_ACT_GELU_ERF.
 * The operand producer of the opt-in parity mode I2T_PRECISE=1 (image2text_amd/ops.py: every GEMM as hi.hi + lo.hi + hi.lo through the
 * accumulate class; inference only, never part of a measured step).  The reference computes these operands in fp32
 * (models/layers.py: nn.Linear on fp32 activations under precision '32'). */
int i2t_split_f32_bf16(void* stream, const float* src, void* hi, void* lo, long n, int act);
/* in-place dropout of x[rows][cols] (f32 or bf16) with the same counter-based keep rule as the fused epilogues:
 * mode 1: element (r, c) kept iff u8(key, r*cols + c) >= thr; mode 2: all of (r, third t of cols) kept iff
 * u8(key + t, r) >= thr (u8 and thr as for i2t_gemm_bf16).  Used for the embedding dropouts and to re-apply a forward mask to a gradient. */
int i2t_dropout_apply(void* stream, void* x, int is_f32, long rows, int cols, int mode, unsigned key, unsigned thr,
                      float scale);
int i2t_adamw_step(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, long n,
                   const long* seg_end, const float* seg_lr, const float* seg_wd, int nseg,
                   float beta1, float beta2, float eps, int step, float grad_scale);
/* SNRAdam (reference models/optimizer.py:56-113; trainer.py:169 `use_snr_optim`): Adam with the gradient's running VARIANCE
 * in the denominator.  Same contract as i2t_adamw_step (frozen segments: lr < 0); a segment at lr == 0 (warm-up from 0) still advances its moments, as the reference does. */
int i2t_snradam_step(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, long n,
                     const long* seg_end, const float* seg_lr, const float* seg_wd, int nseg,
                     float beta1, float beta2, float eps, int step, float grad_scale);
/* y[b][r][:] = src[r][:] for r < rows (broadcast a (rows,d) f32 block into a strided batch buffer) */
int i2t_bcast_rows(void* stream, const float* src, float* y, long y_batch_stride, int B, int rows, int d);
/* ... with the same elementwise dropout on the rows it writes (index b * y_batch_stride + i: they head their slab) */
int i2t_bcast_rows_drop(void* stream, const float* src, float* y, long y_batch_stride, int B, int rows, int d,
                        unsigned drop_key, unsigned drop_thr, float drop_scale);
/* dst[r][:] (+)= sum_b x[b][r][:] */
int i2t_sum_over_batch(void* stream, const float* x, long x_batch_stride, float* dst, int B, int rows, int d,
                       int accumulate);
/* strided f32 row copy with optional bf16 output: y[b][r][:] = x[b][r][:] for r < rows */
int i2t_copy_rows(void* stream, const float* x, long x_bs, void* y, long y_bs, int y_is_bf16, int B, int rows,
                  int d);
int i2t_add_f32(void* stream, float* dst, const float* src, long n);

/* ---------------------------------------------------------------------------------------------------------
 * Greedy decode step pieces (vision_encoder_decoder.py:136-182 with top_k=1, temperature=1):
 *   decode_attention: one new query token per caption against the self K/V cache (keys 0..*pos); head h of caption b starts at
 *     kcache + b * cache_bs + h * cache_hs and its keys are cache_rs apart: cache_hs = 64, cache_rs = d is the token-major layout
 *     [B][Tmax][d] (what a projection GEMM writes: the cross-attention K/V, fixed n_keys, pos_ptr NULL), cache_hs = Tmax * 64,
 *     cache_rs = 64 the head-major layout [B][H][Tmax][64] of the self-attention cache (a head's keys are one contiguous run:
 *     the step is HBM-bound on exactly these reads);
 *     append_dm = d (0 = off): q is a packed [q|k|v] row and the new k/v are written to the cache at *pos by the same
 *     launch (fused kv_append);
 *   ngram_ban_argmax: HF NoRepeatNGramLogitsProcessor for every size in ngram_sizes (prompt included), then argmax
 *     (first index on ties); appends the token at ids[b][*len] and (block 0) bumps *len / *pos after the grid.
 *   Positions live in device memory so that a captured hipGraph replays the same launch for every step.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_decode_attention(void* stream, const void* q, int q_rs, void* kcache, void* vcache,
                         long cache_bs, int cache_rs, long cache_hs, void* o, int o_rs, const int* pos_ptr, int n_keys_fixed,
                         int append_dm, int B, int H);
int i2t_kv_append(void* stream, const void* qkv, int qkv_rs, void* kcache, void* vcache, long cache_bs,
                  int cache_rs, const int* pos_ptr, int B, int d);
/* Prompt prefill of the decode caches (generate_captions(prompt_prefill='pass')): the K and V rows that ONE forward pass over m
 * prompt tokens of B images left in `src` (bf16 rows src_ld apart, K at column k_off, V at v_off, w = Hkv * hd columns each; token t
 * of image b is source row b * src_T + src_t0 + t, t < m) are copied to cache slots slot0 .. slot0 + m - 1 of the N cache rows
 * b * N .. b * N + N - 1 of every image.  Element (row, head, slot, column) of a cache is at row * cache_bs + head * cache_hs +
 * slot * cache_rs + column, as i2t_decode_attention / i2t_gq_decode_attention address it: head-major [R][H][clen][64] is cache_rs =
 * 64, cache_hs = clen * 64; row-major [R][clen][w] is cache_rs = w, cache_hs = hd.  Every 16-byte chunk of a source row is loaded
 * once and stored N times; no other slot and no other cache row is written.  Refused: null pointers, w % 8, hd % 8 (or hd not
 * dividing w), src_ld % 8, column offsets off a multiple of 8 or outside the row, bases off 16 bytes, strides off 8 elements,
 * m < 1, src_t0 + m > src_T, slot0 + m beyond what cache_bs (cache_hs) holds. */
int i2t_kv_prefill(void* stream, const void* src, int src_ld, int k_off, int v_off, int src_T, int src_t0, int m, void* kcache,
                   void* vcache, long cache_bs, int cache_rs, long cache_hs, int hd, int w, int slot0, int B, int N);
int i2t_ngram_ban_argmax(void* stream, const void* logits, int ld, int logits_is_f32, int64_t* ids, int ids_ld,
                         int* len_ptr, const int* ngram_sizes, int n_sizes, int B, int V, float* margin_out);
/* The greedy step's lm_head without its logits (vision_encoder_decoder.py:143-180 with top_k = 1): i2t_gemm_bf16_top2 runs
 * logits = A [M][lda] . B^T (B = the head's rows [N][ldb], bf16, K % 128 == 0) on the persistent GEMM kernel and leaves, for every
 * 64-column segment of a row, its two largest values and their columns -- top2[M][nseg][4] = {v1, column1 (int bits), v2, column2},
 * value descending, lower column first on ties, nseg = ceil(N / 64); i2t_top2_ngram_argmax then applies the n-gram ban and takes the
 * argmax over the segments (a segment whose two leaders are both banned is re-evaluated from `hidden` and `w_head`), writing the token
 * at ids[b][*len_ptr] as i2t_ngram_ban_argmax does.  No margin output: callers that want margins use the logits form. */
int i2t_gemm_bf16_top2(void* stream, const void* A, int lda, const void* B, int ldb, int M, int N, int K, float* top2, int nseg);
int i2t_top2_ngram_argmax(void* stream, const float* top2, int nseg, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d,
                          int64_t* ids, int ids_ld, int* len_ptr, const int* ngram_sizes, int n_sizes, int B, int V);
/* Caption scoring without the logits (an addition: the reference has no such call; it is log_softmax(logits / T) gathered at given
 * labels).  i2t_gemm_bf16_lse runs z = scale . A [M][lda] . B^T (B = the head's rows [N][ldb], bf16, K % 128 == 0) on the persistent GEMM
 * kernel as i2t_gemm_bf16_top2 does and leaves, for every 64-column segment of a row, stats[M][nseg][2] = {mx, se}: mx = max_c z[m][c],
 * se = sum_c exp(z[m][c] - mx) over the segment's columns c < N, nseg = ceil(N / 64) -- 8 bytes per 64 columns, no atomics, bit-
 * reproducible.  i2t_lse_token_logprob merges a row's segments in a fixed order into lse[m] = log sum_c exp(z[m][c]), re-evaluates
 * the label's logit z_t = scale . hidden[m] . w_head[label] in fp32 from the bf16 operands and writes logprob[m] = z_t - lse[m];
 * a row whose label is ignore_index or outside [0, V) gets logprob 0 exactly (its lse is still written). */
int i2t_gemm_bf16_lse(void* stream, const void* A, int lda, const void* B, int ldb, int M, int N, int K, float scale, float* stats, int nseg);
int i2t_lse_token_logprob(void* stream, const float* stats, int nseg, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d,
                          float scale, const int64_t* labels, int64_t ignore_index, float* lse, float* logprob, int M, int V);
int i2t_embed_step(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const float* wte,
                   const float* wpe, float* x, int B, int d, int pos_offset, int vocab);
/* One sampling step of generate() for B captions (reference models/vision_encoder_decoder.py:150-180, the non-greedy modes; the
 * call shape of trainer.py:41-56 eval_model is temperature 0.7 / nucleus 0.6): logits f32 [B][ld] of the last position ->
 * / temperature -> no-repeat-n-gram ban over ids[b][0 .. len) -> top-k crop (top_k <= 0: none; ties at the k-th value stay) ->
 * softmax -> nucleus cut (nucleus_p < 0: none; keeps the sorted prefix whose running sum <= max(nucleus_p, largest probability))
 * -> renormalise -> draw -> ids[b][len] = token.  *len_ptr (device) is the current length; seed = 2 device words.  The draw is
 * the inverse CDF in vocabulary order at u = uniform(seed, len, b) (image2text_amd/rng.py::sample_uniform is the host replica):
 * reproducible per (seed, step, row).  dist_out (optional, f32 [B][dist_ld]) receives the kept, renormalised distribution. */
int i2t_sample_token(void* stream, const float* logits, int ld, int64_t* ids, int ids_ld, const int* len_ptr,
                     const int* ngram_sizes, int n_sizes, int B, int V, float temperature, int top_k, float nucleus_p,
                     const unsigned* seed, float* dist_out, int dist_ld);
int i2t_advance(void* stream, int* counters, int n, int delta);   /* counters[0..n) += delta */
/* The caption step (VisionEncoderDecoder.generate_captions, an addition next to generate()): the three token choosers
 * above in a form that also records the log-probability of the token they choose, and the finish rule.  tok_lp[b][*len_ptr] =
 * z[chosen] - log sum_c exp(z[b][c]) over the whole vocabulary of the step's RAW logits: ban, temperature, crop and nucleus do not
 * enter.  Each takes `done` (a device word) and writes NOTHING once *done is non-zero.  On the same inputs the chosen ids are those of
 * the plain forms, bit for bit.
 *   i2t_gemm_bf16_top2_lse: i2t_gemm_bf16_top2 (top2 bit-equal) that also leaves se[M][nseg], se = sum_c exp(z[m][c] - v1) over the
 *     segment's columns c < N (v1 = the segment's maximum), reduced as i2t_gemm_bf16_lse reduces it; no atomics.
 *   i2t_top2_ngram_argmax_lp: merges a row's (v1, se) pairs in a fixed order into the lse, re-evaluates the chosen logit in fp32.
 *   i2t_ngram_ban_argmax_lp: fp32 logits [B][ld]; the lse is an online pass over the unbanned row.
 *   i2t_sample_token_lp: the raw row's maximum and sum of exp's are taken before the filters.
 *   i2t_caption_finish (after a chooser, before i2t_beam_advance(counters, ctrl)): returns at once if ctrl[0]; a row that finished
 *     earlier gets ids[r][len] = pad and tok_lp[r][len] = 0; else a row with ids[r][len] == eos gets finished[r] = 1 and
 *     lengths[r] = len + 1; ctrl[1] = the number of rows not finished (R when eos < 0: no rule).  One workgroup, no atomics.
 *   i2t_caption_finish_ragged (in its place when the rows' prompts differ in length): row r belongs to image b = r / N
 *     whose prompt is prompt[b][0 .. plen[b]) (prompt int64 [B][prompt_ld], plen int32 [B], both device memory).  While len < plen[b]
 *     the column is FORCED: ids[r][len] = prompt[b][len] over whatever the chooser wrote, tok_lp[r][len] = 0, the row stays unfinished.
 *     From len = plen[b] on the row emits: the rules above, and the row also finishes (lengths[r] = len + 1) with its max_new-th
 *     emitted token, len + 1 - plen[b] >= max_new, whether or not eos >= 0.  ctrl[1] = the rows not finished, forced ones included. */
int i2t_gemm_bf16_top2_lse(void* stream, const void* A, int lda, const void* B, int ldb, int M, int N, int K, float* top2, float* se, int nseg);
int i2t_top2_ngram_argmax_lp(void* stream, const float* top2, const float* se, int nseg, const void* hidden, int ld_hidden,
                             const void* w_head, int ld_w, int d, int64_t* ids, int ids_ld, const int* len_ptr, const int* ngram_sizes,
                             int n_sizes, int B, int V, const int* done, float* tok_lp, int lp_ld);
int i2t_ngram_ban_argmax_lp(void* stream, const float* logits, int ld, int64_t* ids, int ids_ld, const int* len_ptr,
                            const int* ngram_sizes, int n_sizes, int B, int V, const int* done, float* tok_lp, int lp_ld);
int i2t_sample_token_lp(void* stream, const float* logits, int ld, int64_t* ids, int ids_ld, const int* len_ptr,
                        const int* ngram_sizes, int n_sizes, int B, int V, float temperature, int top_k, float nucleus_p,
                        const unsigned* seed, float* dist_out, int dist_ld, const int* done, float* tok_lp, int lp_ld);
int i2t_caption_finish(void* stream, int64_t* ids, int ids_ld, const int* len_ptr, int eos, int64_t pad, int* finished, int* lengths,
                       float* tok_lp, int lp_ld, int* ctrl, int R);
int i2t_caption_finish_ragged(void* stream, int64_t* ids, int ids_ld, const int* len_ptr, const int64_t* prompt, int prompt_ld,
                              const int* plen, int N, int max_new, int eos, int64_t pad, int* finished, int* lengths, float* tok_lp,
                              int lp_ld, int* ctrl, int R);
/* The logits processors of a caption step (generate_captions' repetition_penalty / suppress_tokens / min_new_tokens; DESIGN.md 4s,
 * ABI 11): a pre-pass and a post-pass around the fp32-logits choosers above, which run between them as they are.
 *   i2t_caption_logits_process (after the lm_head GEMM, before the chooser): returns at once if *done.  Per row r of logits f32
 *     [R][ld] (ld >= V, ld % 4 == 0, base on 16 bytes), one workgroup: raw_lse[r] = log sum_c exp(z[r][c]) over the RAW row, reduced in
 *     a fixed order (no atomics); saved[r][j] = the raw z[r][ids[r][j]] for j < len = *len_ptr (saved f32 [R][saved_ld], saved_ld >=
 *     ids_ld); then, in the order of transformers' RepetitionPenalty -> SuppressTokens -> MinNewTokensLength processors, in place:
 *     every token t of ids[r][0 .. len) gets z[t] = z[t] > 0 ? z[t] * inv_theta : z[t] * theta, ONCE however often it occurs
 *     (inv_theta = fp32 1 / theta, formed by the caller: one fp32 multiply per token here); z[t] = -inf for the n_suppress ids of
 *     suppress (int32, device memory; 0 <= n_suppress < V); z[eos] = -inf while len - p < min_new, p = plen[r / N] (int32 [R / N],
 *     device memory) or P when plen is null (eos < 0: no rule).  An id outside [0, V) takes no part.
 *   i2t_caption_raw_logprob (after the chooser, before i2t_caption_finish[_ragged]): returns at once if *done.  With c = ids[r][len]
 *     the chosen token, tok_lp[r][len] = z_raw[c] - raw_lse[r] over what the chooser wrote there, z_raw[c] = saved[r][j] for a j < len
 *     with ids[r][j] == c, else logits[r][c] (a column the pre-pass left raw: a suppressed or min-length-banned token is never
 *     chosen).  So tok_lp keeps the definition above -- the processors do not enter it.  One wave per row. */
int i2t_caption_logits_process(void* stream, float* logits, int ld, const int64_t* ids, int ids_ld, const int* len_ptr, const int* plen,
                               int P, int N, const int* suppress, int n_suppress, int eos, int min_new, float theta, float inv_theta,
                               const int* done, float* raw_lse, float* saved, int saved_ld, int R, int V);
int i2t_caption_raw_logprob(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const float* raw_lse, const float* saved,
                            int saved_ld, const float* logits, int ld, const int* done, float* tok_lp, int lp_ld, int R, int V);
/* The alternatives of a caption step (generate_captions' top_logprobs; DESIGN.md 4ad, ABI 21), after the lm_head GEMM and before
 * anything writes the row.  Per row r of logits f32 [R][ld] (ld >= V, ld % 4 == 0, base on 16 bytes), one workgroup, with len =
 * *len_ptr: top_tok[r][len][j] (int32 [R][out_ld][K]) = the j-th best column of the RAW row z over [0, V) by (z descending, id
 * ascending), exact; top_lp[r][len][j] (f32, same shape) = z[that column] - lse, lse = log sum_c exp(z[c]) with i2t_rows_lse's bits
 * for the row and ONE fp32 subtraction (-inf for a column that holds -inf); entropy[r][len] (f32 [R][out_ld]) = sum_c p_c (lse - z[c]),
 * p_c = exp(z[c] - lse), a -inf column adding 0, reduced in a fixed order (no atomics: bit-reproducible).  1 <= K <= 8, K <= V.
 * Returns at once if *done; writes nothing for a row with finished[r], for a row whose column is still inside its prompt (plen int32
 * [R / N], device memory, non-null and len < plen[r / N]) and when len >= out_ld; else exactly column len of the row's three outputs.
 * Columns [V, ld) are never read.  The row is only read. */
int i2t_caption_top_logprobs(void* stream, const float* logits, int ld, const int* len_ptr, const int* plen, int N, const int* finished,
                             const int* done, int* top_tok, float* top_lp, float* entropy, int out_ld, int K, int R, int V);
/* The same for captions that are GIVEN (VisionEncoderDecoder.score's top_logprobs; DESIGN.md 4ae, ABI 22), behind the fp32 lm_head GEMM
 * of a chunk of teacher-forced rows.  Per row r of logits f32 [R][ld] (ld >= V, ld % 4 == 0, base on 16 bytes), one workgroup, on
 * v[c] = fp32(z[c] * scale), ONE rounded fp32 multiply per column (scale finite and positive; at scale 1 v is z): top_tok[r][j] (int32
 * [R][K]) = the j-th best column over [0, V) by (v descending, id ascending), exact; top_lp[r][j] (f32 [R][K]) = v[that column] -
 * lse[r] in ONE fp32 subtraction (-inf for a column that holds -inf); lse[r] = log sum_c exp(v[c]) in i2t_rows_lse's order -- at
 * scale 1 its bits for the row --; entropy[r] = sum_c p_c (lse - v[c]), p_c = exp(v[c] - lse), a -inf column adding 0, reduced in a
 * fixed order.  With y = labels[r] (int64 [R], device memory): rank[r] (int32) = the number of columns strictly ahead of y in that
 * order -- 0: y is the arg-max; where rank[r] < K, top_tok[r][rank[r]] == y -- and logprob[r] = v[y] - lse[r], the same bits as
 * top_lp[r][rank[r]] there, -inf where column y holds -inf.  y == ignore_index or outside [0, V): rank -1, logprob 0.0; the row's
 * other outputs are written all the same.  1 <= K <= 8, K <= V, R > 0.  No atomics: two launches give the same bits.  Columns
 * [V, ld) are never read.  The rows are only read; a refused call writes nothing. */
int i2t_score_top_logprobs(void* stream, const float* logits, int ld, float scale, const int64_t* labels, int64_t ignore_index, int* top_tok,
                           float* top_lp, float* entropy, int* rank, float* lse, float* logprob, int K, int R, int V);
/* Closed-set decoding (generate_captions' phrases; DESIGN.md 4u, ABI 13): every row emits one phrase of a set and then EOS.  The set is
 * a flat CSR trie in device memory, all int32: the children of node n are edges child_off[n] .. child_off[n + 1) (child_off [nodes + 1]),
 * child_tok [edges] ascending within a node, child_next [edges] the node an edge leads to, term [nodes] the index of the phrase that
 * ends at the node or -1; node 0 is the root; node [R] holds every row's node.  `nodes` and `edges` are what the arrays hold: the
 * kernels clip every index to them.  A pre-pass and a post-pass around the fp32-logits choosers above, which run between them as they
 * are (with no n-gram sizes).  Bases on 16 bytes; ld >= V, ld % 4 == 0; 0 <= eos < V.
 *   i2t_caption_trie_mask (after the lm_head GEMM, before the chooser): returns at once if *done.  Per row r of logits f32 [R][ld], one
 *     workgroup: raw_lse[r] = log sum_c exp(z[r][c]) over the RAW row, reduced in a fixed order (no atomics); kept[r][i] = the raw
 *     z[r][child_tok[off + i]] for the fan children of node[r] and kept[r][fan] = z[r][eos] when term[node[r]] >= 0 (kept f32
 *     [R][kept_ld], kept_ld >= the largest fan-out + 1); then columns [0, V) of the row hold -inf except the children's and, at such a
 *     node, the EOS column, which hold their raw values.  Columns V .. ld are not touched.  Any fan-out from 1 to V - 1.
 *   i2t_caption_trie_advance (after the chooser, before i2t_caption_finish): returns at once if *done; a row with finished[r] is
 *     skipped.  With c = ids[r][len]: c == eos at a node with term >= 0 sets phrase_index[r] = term[node[r]]; a child of the node sets
 *     node[r] = its child_next; in both cases tok_lp[r][len] = logits[r][c] - raw_lse[r], the raw row's log_softmax at c, over what the
 *     chooser wrote there.  Any other token leaves node, phrase_index and tok_lp as they were.  One wave per row. */
int i2t_caption_trie_mask(void* stream, float* logits, int ld, const int* node, const int* child_off, const int* child_tok,
                          const int* term, int nodes, int edges, int eos, const int* done, float* raw_lse, float* kept, int kept_ld,
                          int R, int V);
int i2t_caption_trie_advance(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const int* finished,
                             const float* logits, int ld, const float* raw_lse, const int* child_off, const int* child_tok,
                             const int* child_next, const int* term, int nodes, int edges, int eos, const int* done, int* node,
                             int* phrase_index, float* tok_lp, int lp_ld, int R, int V);
/* Exact closed-set scoring (score_phrases; DESIGN.md 4v, ABI 14): the log-likelihood of EVERY phrase of a set, the trie walked level by
 * level with every node of a level a row (W rows per image, row b * W + w) and nothing pruned.  The level tables are host-built, static
 * and int32; bases on 16 bytes.
 *   i2t_rows_lse: lse[r] = log sum_c exp(logits[r][c]) over columns [0, V) of logits f32 [R][ld] (ld >= V, ld % 4 == 0), one workgroup
 *     per row in i2t_caption_trie_mask's reduction order (no atomics, bit-reproducible); the rows are only read.
 *   i2t_trie_level_expand, one wave per (image, entry), after the level's step and its rows' lse.  Child part, entry j < n_child: the
 *     next level's row b W + j takes token k = child_tok[j] behind the parent in row p = child_parent[j] (0 <= p < W) of this level:
 *     path_out[b W + j] = path_in[b W + p] + (z - lse[b W + p]) in this order in fp32, ids[b W + j][*len_ptr] = k.  Terminal part,
 *     entry j < n_term: row p = term_row[j] holds a node that ends a phrase; every phrase index i of term_phrase[term_off[j] ..
 *     term_off[j + 1]) (term_off [n_term + 1], term_phrase [n_term_phrases]) gets logprob[b][i] = path_in[b W + p] + (z_eos - lse[b W + p])
 *     (logprob f32 [B][lp_ld]).  z = logits[b W + p][k] when `logits` is given (f32 [B W][ld]); else scale . hidden[b W + p] .
 *     w_head[k], re-evaluated in fp32 from the bf16 operands as i2t_lse_token_logprob does (d % 8 == 0, rows on 16 bytes).  path_in and
 *     path_out are two buffers.  Nothing else is written; an entry whose parent row or token is outside its range writes nothing (the
 *     host checks the tables before upload).  n_child = n_term = 0 launches nothing. */
int i2t_rows_lse(void* stream, const float* logits, int ld, float* lse, int R, int V);
int i2t_trie_level_expand(void* stream, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d, float scale,
                          const float* logits, int ld, const float* lse, const float* path_in, float* path_out,
                          const int* child_parent, const int* child_tok, int n_child, const int* term_row, const int* term_off,
                          const int* term_phrase, int n_term, int n_term_phrases, int64_t* ids, int ids_ld, const int* len_ptr,
                          float* logprob, int lp_ld, int eos, int B, int W, int V);
/* i2t_trie_level_expand with a phrase set and a prompt length per image (score_phrases' phrase_sets; DESIGN.md 4ab, ABI 19): the
 * images of one launch stand at different levels of different tries, in a forced prompt column, or behind their last level.  The level
 * tables of every (set, level) lie end to end: child_parent / child_tok [n_child_all], term_row [n_term_all], term_off [n_off_all]
 * (each level's n_term + 1 offsets; they index term_phrase [n_term_phrases] absolutely).  image_state int32 [B][8] (device memory,
 * base on 16 bytes, host-built per step) holds per image: 0 the level, or -1; 1 the forced token, or -1; 2 / 3 where its level's
 * children start in child_parent / child_tok and how many they are; 4 / 5 the same for term_row; 6 where its level's offsets start
 * in term_off; 7 the id column it writes.  One wave per (image, entry), the child part over e_child and the terminal part over e_term
 * entries per image (each 0 .. W).
 *   level -1 with a forced token k in [0, V): ids[b W + j][column] = k and path_out[b W + j] = path_in[b W + j] for j < W (the child
 *     part; e_child must reach W for such an image); nothing is scored.  Level -1 and token -1: the image is finished, nothing of it
 *     is read or written.
 *   level >= 0: entry j of the image's own ranges does what i2t_trie_level_expand does with entry j of its tables, the arithmetic
 *     operation for operation (one device function); the terminal part writes logprob[b][i], i < kmax <= lp_ld.
 * Refused before any launch: what i2t_trie_level_expand refuses; a null or misaligned image_state; negative table sizes, fewer
 * offsets than terminal rows + 1; e_child or e_term outside 0 .. W; kmax outside 1 .. lp_ld.  What image_state HOLDS is device memory:
 * the host checks it before upload, and the kernel writes nothing for an entry outside its image's range, a range outside the tables,
 * a parent row outside [0, W), a token outside [0, V), a phrase index outside [0, kmax) or a column outside [0, ids_ld). */
int i2t_trie_level_expand_sets(void* stream, const void* hidden, int ld_hidden, const void* w_head, int ld_w, int d, float scale,
                               const float* logits, int ld, const float* lse, const float* path_in, float* path_out,
                               const int* child_parent, const int* child_tok, int n_child_all, const int* term_row, int n_term_all,
                               const int* term_off, int n_off_all, const int* term_phrase, int n_term_phrases, const int* image_state,
                               int e_child, int e_term, int64_t* ids, int ids_ld, float* logprob, int lp_ld, int kmax, int eos, int B,
                               int W, int V);
/* Beam search over the phrase trie (search_phrases; DESIGN.md 4w, ABI 15): the N best phrases of a set, W <= 8 rows per image (row
 * b * W + w) whatever the size of the set; every row holds a trie node (node int32 [R], -1 or anything outside [0, nodes): a dead row) and
 * an fp32 path sum (path [R]).  The trie is the CSR trie above, `nodes` and `edges` what its arrays hold.  No atomics, fixed reduction
 * orders: both kernels are bit-reproducible.  decoding_host.trie_beam_candidates_host / trie_beam_select_host state them on the host.
 *   i2t_trie_beam_candidates (after the fp32 lm_head), one workgroup per row: returns at once if ctrl[0].  Per live row of logits f32
 *     [R][ld] (ld >= V, ld % 4 == 0, bases on 16 bytes): lse = log sum_c exp(z[c]) over the RAW row in i2t_rows_lse's order, bit-equal to
 *     that entry point (written to lse[r] when `lse` is given); fin_total[r] = path[r] + (z[eos] - lse) when term[node[r]] >= 0, else
 *     -inf; every edge e of the node has total = path[r] + (z[child_tok[e]] - lse), in this order in fp32, and cand_edge [R][W] /
 *     cand_total [R][W] take the W largest, descending, the lower edge first on ties (-1 / -inf where the node has fewer than W
 *     children).  A dead row writes -1 / -inf / -inf and reads no logits.  Any fan-out from 0 to V - 1.  1 <= W <= 8, 0 <= eos < V.
 *   i2t_trie_beam_select, one workgroup per image: returns at once if ctrl[0] or closed[b]; with t = *len_ptr - P outside 0 .. longest,
 *     *len_ptr >= ids_ld or *pos_ptr outside [0, hist_ld) nothing is written.  In row order, a live row whose node ends a phrase offers
 *     (term[node], f = fin_total, s = f / powf(t + 1, length_penalty), t + 1) to the image's pool pool_phrase / pool_sum / pool_score /
 *     pool_len [B][W] (pool_n [B] entries, descending by score): the pool keeps the W best, an entry it holds before a new one of equal
 *     score.  The W largest candidates of the image's rows (descending, the lower row first, then the lower edge on ties) become rows
 *     0 .. of the image: node = child_next[e], path = the total, ids[row][*len_ptr] = child_tok[e], hist[row][*pos_ptr] = the parent's
 *     row behind the parent's history columns [0, *pos_ptr); a row without a candidate is dead: node -1, path -inf, token eos, its own
 *     history row.  closed[b] = 1 when no row is live, or when the pool holds W and not (best next total / powf(Lopt, length_penalty) >
 *     pool_score[b][W - 1]), Lopt = longest + 1 for a penalty >= 0, else t + 2; an image left open stores 1 into ctrl[1].
 *     i2t_beam_advance moves the counters.  1 <= W <= 8, P >= 1, longest >= 1, P + longest + 1 <= ids_ld, a finite length_penalty. */
int i2t_trie_beam_candidates(void* stream, const float* logits, int ld, const int* node, const float* path, const int* child_off,
                             const int* child_tok, const int* term, int nodes, int edges, int eos, const int* ctrl, int* cand_edge,
                             float* cand_total, float* fin_total, float* lse, int R, int W, int V);
int i2t_trie_beam_select(void* stream, const int* cand_edge, const float* cand_total, const float* fin_total, int* node, float* path,
                         const int* child_tok, const int* child_next, const int* term, int nodes, int edges, int eos, int64_t* ids, int ids_ld,
                         int* hist, int hist_ld, int* pool_phrase, float* pool_sum, float* pool_score, int* pool_len, int* pool_n, int* closed,
                         const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W, int P, int longest, float length_penalty);

/* A prompt length and a phrase set per image (generate_captions' / search_phrases' phrase_sets; DESIGN.md 4x, ABI 16).  The sets' tries
 * lie end to end in the CSR arrays above (phrase_trie.phrase_forest): the kernels index nodes blindly, so a row that starts at its
 * set's root never leaves that set, and term holds the phrase index WITHIN the set.  The start nodes are the caller's (no kernel).
 *   i2t_caption_trie_mask_ragged / i2t_caption_trie_advance_ragged: the two kernels above with row r belonging to image r / N (R % N
 *     == 0, N >= 1) whose prompt is plen[r / N] long (int32 [R / N], device memory, base on 16 bytes).  While *len_ptr < plen[r / N]
 *     the row sits in a forced column: the mask leaves its logits row raw and writes neither raw_lse[r] nor kept[r]; the advance
 *     leaves node[r], phrase_index[r] and tok_lp[r][len].  The chooser still runs on the row; i2t_caption_finish_ragged replaces its
 *     token and log-prob afterwards.  Every other row: exactly the kernels above.
 *   i2t_trie_beam_select_sets: i2t_trie_beam_select with plen int32 [B] and longest_of int32 [B] (device memory, bases on 16 bytes) in
 *     place of the scalars; plen null: every image's prompt is P long (with plen given the kernel does not read P; the entry point
 *     still holds it to 1 <= P and P + 2 <= ids_ld, so pass the longest prompt).  For image b, t = *len_ptr - plen[b].  t < 0 is a forced
 *     column: pool, node, path, closed and ids are not touched (the caller put the prompt into ids), hist[b W + w][*pos_ptr] = b W + w
 *     for every row and the image stores 1 into ctrl[1].  t >= 0: the rule above with longest_of[b] in the guard, the close test and
 *     the column bound.  No id column at or past ids_ld and no history column outside [0, hist_ld) is written whatever the tables
 *     hold.  i2t_trie_beam_candidates runs unchanged on all rows; a forced image's candidates are ignored.  P >= 1, P + 2 <= ids_ld. */
int i2t_caption_trie_mask_ragged(void* stream, float* logits, int ld, const int* node, const int* child_off, const int* child_tok,
                                 const int* term, int nodes, int edges, int eos, const int* done, float* raw_lse, float* kept, int kept_ld,
                                 const int* len_ptr, const int* plen, int N, int R, int V);
int i2t_caption_trie_advance_ragged(void* stream, const int64_t* ids, int ids_ld, const int* len_ptr, const int* finished,
                                    const float* logits, int ld, const float* raw_lse, const int* child_off, const int* child_tok,
                                    const int* child_next, const int* term, int nodes, int edges, int eos, const int* done, int* node,
                                    int* phrase_index, float* tok_lp, int lp_ld, const int* plen, int N, int R, int V);
int i2t_trie_beam_select_sets(void* stream, const int* cand_edge, const float* cand_total, const float* fin_total, int* node, float* path,
                              const int* child_tok, const int* child_next, const int* term, int nodes, int edges, int eos, int64_t* ids,
                              int ids_ld, int* hist, int hist_ld, int* pool_phrase, float* pool_sum, float* pool_score, int* pool_len,
                              int* pool_n, int* closed, const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W, int P,
                              const int* plen, const int* longest_of, float length_penalty);

/* -----------------------------------------------------------------------------------------------------------
 * The nano-mini block family (reference training_configs/gpu/nano-mini.yaml).
 *
 * Grouped-query attention, head_dim 16 / 32 / 64 / 128 (reference models/layers.py:391-430 MultiQueryAttention = H query heads
 * on ONE shared key/value head, Hkv = 1; Hkv = H is multi-head attention at widths i2t_attention_* does not cover, i.e.
 * nn.MultiheadAttention with 128-wide heads, layers.py:537-542).  Same conventions as i2t_attention_fwd / _bwd (strides, packed
 * rows, lse layout, causal rule, dropout index space, out_drop multipliers); query head h starts at column hd*h of q / o / dq,
 * key/value head h / (H / Hkv) at column hd*(h / (H / Hkv)) of k / v / dk / dv; dk / dv hold the SUM over the query heads that
 * share a key/value head. */
int i2t_gq_attention_fwd(void* stream, const void* q, long q_bs, int q_rs, const void* k, long k_bs, int k_rs,
                         const void* v, long v_bs, int v_rs, void* o, long o_bs, int o_rs, float* lse,
                         int B, int H, int Hkv, int hd, int Tq, int Tk, int causal,
                         unsigned drop_key, unsigned drop_thr, float drop_scale,
                         const int* cu_q, const int* cu_k, int total_q, int split);
/* split (forward only, dense non-causal self-attention; 0 = off): query rows >= split do not see keys < split -- the mask of a
 * NON-causal decoder over [soft prompt | text] (reference models/vision_encoder_decoder.py:93-99,106-113: prompt rows see every
 * column, text rows never see the prompt columns). */
int i2t_gq_attention_bwd(void* stream, const void* q, long q_bs, int q_rs, const void* k, long k_bs, int k_rs,
                         const void* v, long v_bs, int v_rs, const void* o, long o_bs, int o_rs,
                         const void* d_o, long do_bs, int do_rs, const float* lse, float* delta_ws,
                         void* dq, long dq_bs, int dq_rs, void* dk, long dk_bs, int dk_rs,
                         void* dv, long dv_bs, int dv_rs, int B, int H, int Hkv, int hd, int Tq, int Tk, int causal,
                         unsigned drop_key, unsigned drop_thr, float drop_scale,
                         const int* cu_q, const int* cu_k, int total_q,
                         unsigned out_drop_key, unsigned out_drop_thr, float out_drop_scale);
/* x[m][n] *= keep(key0 + n / section, m) ? scale : 0 on a bf16 [rows][ld] matrix: the per-token q / k / v multipliers of
 * layers.py:412-420 on the separate q_proj (section = d, key0 = key) and kv_proj (section = hd, key0 = key + 1) outputs. */
int i2t_row_sections_dropout(void* stream, void* x, int ld, long rows, int cols, int section, unsigned key0, unsigned thr, float scale);

/* Sparse token subsets (layers.py:570-577, 609-614): out[i][:] = src[idx[i]][:] (fp32 and / or bf16 copy), dst[idx[i]][:] = src[i][:]. */
int i2t_gather_rows(void* stream, const float* src, const int* idx, float* out_f32, void* out_bf16, long n, int d);
int i2t_scatter_rows(void* stream, const float* src, const int* idx, float* dst, long n, int d);

/* MoELinear routing (layers.py:330-346).  U f32 [M][ldu] = x [l1_0; ..; l1_{E-1}; gate layer 0]^T + bias: columns [0, E P) the
 * experts' pre-activations, then G gate-hidden pre-activations (G > 0: gate = Linear-GELU-Linear, wg2 f32 [E][G], bg2 f32 [E] or
 * null) or the E gate logits themselves (G = 0).  gates = softmax(logits * inv_sqrt_in); the top_k largest are the routing
 * weights w (not renormalised), all others 0.  A bf16 [M][Kp] = [w_e gelu(U[e P + j]) | w_0 .. w_{E-1} | 0 pad] is the left
 * operand of y = A W2aug^T (i2t_moe_pack_w2).  gates / wsel f32 [M][E] are kept for the backward pass.
 * bwd: dA bf16 [M][Kp] = dy W2aug -> D1 bf16 [M][ldd] = dL/dU (pad columns zeroed), dwg2 / dbg2 += the gate's second layer
 * gradients (fixed summation order; part_ws f32 [i2t_moe_gate_bwd_blocks(M)][E G + E]). */
int i2t_moe_gate_fwd(void* stream, const float* U, int ldu, const float* wg2, const float* bg2, void* A, int Kp, float* gates,
                     float* wsel, int M, int E, int P, int G, int top_k, float inv_sqrt_in);
int i2t_moe_gate_bwd_blocks(int M);
int i2t_moe_gate_bwd(void* stream, const void* dA, int Kp, const float* U, int ldu, const float* gates, const float* wsel,
                     const float* wg2, void* D1, int ldd, float* dwg2, float* dbg2, float* part_ws, int M, int E, int P, int G,
                     int top_k, float inv_sqrt_in);
/* W2aug bf16 [out][Kp] = [l2_0.weight | .. | l2_{E-1}.weight | l2_0.bias .. l2_{E-1}.bias | 0] from the stacked parameters
 * l2w bf16 [E][out][P], l2b f32 [E][out]; unpack adds a gradient dW f32 [out][Kp] back onto gw f32 [E][out][P], gb f32 [E][out]. */
int i2t_moe_pack_w2(void* stream, const void* l2w, const float* l2b, void* W, int out, int E, int P, int Kp);
int i2t_moe_unpack_dw2(void* stream, const float* dW, float* gw, float* gb, int out, int E, int P, int Kp);

/* Decode step of the family (static KV cache under hipGraph, see i2t_decode_attention): the new query row q [B][H hd] against the
 * cached keys 0 .. *pos_ptr of its key/value head (Hkv heads of width hd in the cache rows); k_new / v_new [B][>= Hkv hd] are this
 * token's key / value, written to cache slot *pos_ptr and attended to; null k_new / v_new: a fixed memory of n_keys_fixed keys
 * (cross-attention).  max_keys bounds *pos_ptr + 1 (<= 1024). */
int i2t_gq_decode_attention(void* stream, const void* q, int q_rs, const void* k_new, const void* v_new, int kv_rs, void* kcache,
                            void* vcache, long cache_bs, int cache_rs, void* out, int out_rs, const int* pos_ptr,
                            int n_keys_fixed, int max_keys, int B, int H, int Hkv, int hd);
/* i2t_gq_decode_attention for caches past 1024 keys (hd 64 or 128): the keys of a row are split into chunks of CH = LONG_CHUNK_KEYS
 * (csrc/common.h, 256), one wave per (query head, row, chunk), and a second launch combines the chunk results in chunk order, so the
 * output is bit-reproducible.  The grid depends on max_keys only -- the key count *pos_ptr + 1 (or n_keys_fixed) is read on the
 * device and must not exceed max_keys -- so one captured launch pair serves every position.
 *   stream                  HIP stream of both launches
 *   q, q_rs                 bf16 [B][H hd] query rows, row stride q_rs elements
 *   k_new, v_new, kv_rs     bf16 [B][>= Hkv hd] this token's key / value rows (row stride kv_rs): written to cache slot *pos_ptr and
 *                           attended to; both null: nothing is appended, all keys come from the cache
 *   kcache, vcache          bf16 row-major caches, element (row, slot, column) at row * cache_bs + slot * cache_rs + column (16-byte
 *   cache_bs, cache_rs      aligned, strides multiples of 8); every row holds at least max_keys slots
 *   out, out_rs             bf16 [B][H hd] result rows (16-byte aligned, out_rs % 8 == 0)
 *   pos_ptr, n_keys_fixed   device int32: the new token's slot, key count *pos_ptr + 1; null: n_keys_fixed keys (<= max_keys)
 *   max_keys                1 .. 32768 (DECODE_LONG_MAX_KEYS): sizes the grid, NC = ceil(max_keys / CH) chunks per row and head
 *   B, H, Hkv, hd           rows, query heads, key/value heads (H % Hkv == 0), head width
 *   ws, ws_floats           fp32 workspace, 16-byte aligned, at least B * H * NC * (hd + 2) floats: the chunks' unnormalised sums
 *                           [B][H][NC][hd], then their (maximum, sum of exp) pairs [B][H][NC][2]; overwritten by every call
 * The beam form reads key t of row r from cache row hist[r][t] (int32 [R][hist_ld], hist_ld >= max_keys, required; the new token goes
 * to the row's own slot); it has no slot_pos and no rows_per_mem.  With an identity table its output is bit-equal to the plain form's.
 * Every violated bound above is I2T_EINVAL with a message naming the argument, before anything is launched. */
int i2t_gq_decode_attention_long(void* stream, const void* q, int q_rs, const void* k_new, const void* v_new, int kv_rs, void* kcache,
                                 void* vcache, long cache_bs, int cache_rs, void* out, int out_rs, const int* pos_ptr, int n_keys_fixed,
                                 int max_keys, int B, int H, int Hkv, int hd, float* ws, long ws_floats);
int i2t_beam_gq_decode_attention_long(void* stream, const void* q, int q_rs, const void* k_new, const void* v_new, int kv_rs,
                                      void* kcache, void* vcache, long cache_bs, int cache_rs, void* out, int out_rs, const int* pos_ptr,
                                      int n_keys_fixed, int max_keys, const int* hist, int hist_ld, int R, int H, int Hkv, int hd,
                                      float* ws, long ws_floats);
/* Beam-search step over the static KV cache (reference models/generation_utils.py:10-148, BeamSearchTokenGenerator; csrc/beam.hip,
 * the two attention entry points beside their greedy twins in csrc/decode.hip and csrc/family.hip).
 * R = B * W rows, batch-major (row r = b * W + w).  *len_ptr, *pos_ptr and ctrl = [done, unfinished] (int32) live in device memory,
 * so one captured hipGraph replays the step per token; once ctrl[0] is set, candidates / consolidate / advance do nothing.
 *   beam_candidates: logits f32 [R][ld] (ld % 4 == 0, 16-byte aligned) of the last position -> no-repeat-n-gram ban over
 *     ids[r][0 .. len) (prompt included) -> top-k crop (top_k <= 0: none; ties at the k-th value stay) -> E candidates: temperature
 *     <= 0 the E largest scores (descending, lower id first on ties) with log_softmax(scores); else E draws without replacement from
 *     softmax(scores / T) (Gumbel-top-E over uniform(seed, len, r, token, 0): image2text_amd/rng.py::beam_uniform) with
 *     log_softmax(scores / T).  EOS rule (eos >= 0 only): a row whose last token is eos re-emits eos at 0 where lp + log_boost < 0,
 *     every other candidate gets + log_boost.  Writes cand_tok int [R][E], cand_lp f32 [R][E]; raw_tok (optional, [R][E]): the
 *     draws before the EOS rule.  E <= 16.
 *   beam_consolidate: per caption the W survivors of the W * E totals scores[r] + cand_lp (temperature <= 0: the top W, descending,
 *     lower flat index w * E + e first on ties; else W draws without replacement from softmax(total / T) over uniform(seed, len, b,
 *     flat, 1)).  Child b * W + k gets the parent's ids [0 .. len) and history [0 .. pos), ids[child][len] = token, hist[child][pos] =
 *     parent, the new score, parent[child] and has_eos[child] (int [R]: the row holds eos anywhere); ctrl[1] counts the captions
 *     with a beam that has no eos (every caption when eos < 0).  raw_pick (optional, int [R]): the flat index each child was made
 *     from.  W <= 16, W * E <= 1024.
 *   beam_pool_select (generate_captions(num_beams = W); in beam_consolidate's place, after beam_candidates with
 *     temperature <= 0, E = 2 W, eos = -1): one workgroup per image, no atomics; returns at once if ctrl[0], and for an image whose
 *     closed[b] is set.  Ranks the top 2 W of the image's W * 2 W totals scores[r] + cand_lp (descending, lower flat index first).  A
 *     candidate HITS if its token is eos (eos < 0: never) or it is the max_new-th emitted token (emitted = *len_ptr + 1 - P).  Hits
 *     ranked below W are offered to the pool at total / powf((float)emitted, length_penalty), fp32; the pool (pool_ids int64
 *     [B][W][ids_ld], pool_lp f32 [B][W][lp_ld], pool_score / pool_sum f32 [B][W], pool_len int [B][W], pool_n int [B]) keeps the W
 *     best, sorted descending, an entry it holds before a new one on ties; a new row is the parent's ids / tok_lp columns [0, len),
 *     the token and its log-prob at column len, then pad / 0.0 up to column P + max_new; pool_sum is the total, pool_len = len + 1.
 *     The first W candidates that do not hit become rows b * W + k: the parent's ids, tok_lp [0, len) and history [0, pos) move to
 *     the child, ids[child][len] = token, tok_lp[child][len] = its log-prob, hist[child][pos] = parent, scores[child] = total.
 *     closed[b] is set at the bound (the rows then stay as they are), with early_stopping once pool_n[b] = W, and without it once
 *     pool_n[b] = W and not (scores[b * W] / powf((float)emitted, length_penalty) > pool_score[b][W - 1]).  Every image left open
 *     stores 1 into ctrl[1] (a flag, not a count: no atomic).  W <= 8; P + max_new <= ids_ld, lp_ld; counters outside
 *     P <= len < P + max_new, 0 <= pos < hist_ld write nothing.
 *   beam_advance: while ctrl[0] is clear: pos += 1, len += 1, and ctrl[0] = (ctrl[1] == 0); then ctrl[1] = 0.
 *   beam_decode_attention / beam_gq_decode_attention: i2t_decode_attention / i2t_gq_decode_attention with key t of row r read from
 *     cache row hist[r][t] (int32 [R][hist_ld]; the new token's key / value are written to the row's own slot *pos); hist NULL: row
 *     r / rows_per_mem for every key (cross-attention over a memory stored once per image).  Same loads and reduction order: with
 *     an identity table the outputs are bit-equal to the plain kernels'.  beam_gq_decode_attention's slot_pos (int32 [max_keys],
 *     NULL: slot = position; needs hist): the cache of a sparse layer holds its kept positions only, slot s the text position
 *     slot_pos[s], so key s of row r is read from row hist[r][slot_pos[s]]; every entry must be below hist_ld. */
int i2t_beam_candidates(void* stream, const float* logits, int ld, const int64_t* ids, int ids_ld, const int* len_ptr, const int* ctrl,
                        const int* ngram_sizes, int n_sizes, int R, int V, int E, float temperature, int top_k, int eos, float log_boost,
                        const unsigned* seed, int* cand_tok, float* cand_lp, int* raw_tok);
int i2t_beam_consolidate(void* stream, const int* cand_tok, const float* cand_lp, float* scores, int64_t* ids, int ids_ld, int* hist,
                         int hist_ld, int* has_eos, int* parent, const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W, int E,
                         float temperature, int eos, const unsigned* seed, int* raw_pick);
int i2t_beam_pool_select(void* stream, const int* cand_tok, const float* cand_lp, float* scores, int64_t* ids, int ids_ld, int* hist,
                         int hist_ld, float* tok_lp, int lp_ld, int64_t* pool_ids, float* pool_lp, float* pool_score, float* pool_sum,
                         int* pool_len, int* pool_n, int* closed, const int* pos_ptr, const int* len_ptr, int* ctrl, int B, int W, int P,
                         int max_new, int eos, int pad, float length_penalty, int early_stopping);
int i2t_beam_advance(void* stream, int* counters, int* ctrl);
int i2t_beam_decode_attention(void* stream, const void* q, int q_rs, void* kcache, void* vcache, long cache_bs, int cache_rs,
                              long cache_hs, void* o, int o_rs, const int* pos_ptr, int n_keys_fixed, int append_dm, const int* hist,
                              int hist_ld, int rows_per_mem, int R, int H);
int i2t_beam_gq_decode_attention(void* stream, const void* q, int q_rs, const void* k_new, const void* v_new, int kv_rs, void* kcache,
                                 void* vcache, long cache_bs, int cache_rs, void* out, int out_rs, const int* pos_ptr, int n_keys_fixed,
                                 int max_keys, const int* hist, int hist_ld, const int* slot_pos, int rows_per_mem, int R, int H,
                                 int Hkv, int hd);
/* Cross-attention over a memory stored once per image, with a row -> memory-row table (``image_index`` of the decoding calls; DESIGN.md
 * 4ac, ABI 20): row r of the R query rows attends to the n_keys keys of memory row mem_index[r] (int32 [R] on the device).  kmem / vmem:
 * [n_mem][n_keys] rows mem_rs apart, memory rows mem_bs apart; mem_decode_attention: H heads of 64, head h at column h * 64
 * (i2t_decode_attention's token-major layout, cache_hs = 64); mem_gq_decode_attention: Hkv key/value heads of width hd (16, 32, 64,
 * 128) under H query heads (i2t_gq_decode_attention's layout).  No append, no position pointer, no history table, no slot_pos.  The
 * table word is wave-uniform: it is loaded once per workgroup and folded into the base pointers; loads, lanes and reduction order are
 * those of i2t_decode_attention / i2t_gq_decode_attention, so the output is bit-equal to theirs on the gathered memory, and with
 * mem_index[r] = r / W to the beam forms' with rows_per_mem = W.  THE VALUES OF mem_index ARE NOT CHECKED: the caller validates
 * 0 <= mem_index[r] < n_mem on the host before it uploads the table (caption_plan.check_image_index); the kernels do not scan it, and
 * n_mem only takes part in the checks.  I2T_EINVAL with a message, before anything is launched: a null operand, a null mem_index,
 * n_keys outside 1 .. 1024, n_mem < 1, rows that are not 16-byte aligned or too short for their heads, a head width outside the list. */
int i2t_mem_decode_attention(void* stream, const void* q, int q_rs, const void* kmem, const void* vmem, long mem_bs, int mem_rs, void* o,
                             int o_rs, int n_keys, const int* mem_index, int n_mem, int R, int H);
int i2t_mem_gq_decode_attention(void* stream, const void* q, int q_rs, const void* kmem, const void* vmem, long mem_bs, int mem_rs, void* out,
                                int out_rs, int n_keys, const int* mem_index, int n_mem, int R, int H, int Hkv, int hd);
/* Sparse blocks in the decode step: a layer's cache holds only its kept positions, so the token at text position *pos_ptr uses
 * slot rank[l][pos] (= kept positions before it) and runs the block only when member[l][pos]; both tables int [L][tmax] on the
 * device.  setup writes lpos[l] / lmem[l] for the current position; i2t_select_rows picks the block's or the null connector's
 * output (out = *flag ? a : b, fp32 [n]). */
int i2t_sparse_step_setup(void* stream, const int* pos_ptr, const int* rank, const int* member, int* lpos, int* lmem, int L, int tmax);
int i2t_select_rows(void* stream, const int* flag, const float* a, const float* b, float* out, long n);

/* -----------------------------------------------------------------------------------------------------------
 * Llama-2 / Qwen2 decoder blocks (reference models/decoder.py:404-440: Llama2HuggingfaceDecoder / Qwen2HuggingfaceDecoder wrap
 * transformers' LlamaForCausalLM / Qwen2ForCausalLM, a go-through dependency -- transformers 5.x models/llama/modeling_llama.py:
 * LlamaRMSNorm, apply_rotary_pos_emb with rotate_half, LlamaMLP).  Projections are i2t_gemm_bf16, attention
 * is i2t_gq_attention_* (H query heads on Hkv key/value heads).
 *
 * RMSNorm: y (bf16) / y_f32 [M][d] = w * x * rstd (either output may be null), rstd[m] = rsqrt(mean(x[m]^2) + eps) (fp32 x; rstd
 * may be null).  Backward:
 * dx (+)= rstd (dy w - xh mean(dy w xh)), xh = x rstd; dw += sum_m dy xh (null: skipped); dx_bf16 (nullable) = bf16 copy of the
 * dx written (the next GEMM's operand). */
int i2t_rmsnorm_fwd(void* stream, const float* x, const float* w, void* y, float* y_f32, float* rstd, int M, int d, float eps);
int i2t_rmsnorm_bwd(void* stream, const void* dy, int dy_is_f32, const float* x, const float* w, const float* rstd,
                    float* dx, int dx_accumulate, void* dx_bf16, float* dw, int M, int d);
/* Rotary position embedding in place on n_heads heads of width hd starting at column col0 of the bf16 rows x [M][rs]:
 * [x1 | x2] -> [x1 cos - x2 sin | x2 cos + x1 sin] (halves of the head; transformers' rotate_half convention).  cos_sin fp32
 * [n_positions][hd] = [cos(p f_i), i < hd/2 | sin(p f_i)].  Position of row m: pos[m] (packed rows) | *pos_ptr + pos_offset (decode
 * step under hipGraph) | pos_offset + m % T.  inverse != 0 rotates by the negative angle (= the backward of the forward). */
int i2t_rope(void* stream, void* x, int rs, int col0, int n_heads, int hd, const float* cos_sin, int n_positions,
             const int* pos, const int* pos_ptr, int pos_offset, int T, int M, int inverse);
/* SwiGLU on the fused projection gate_up bf16 [M][ld] = [gate (ff) | up (ff)]: h [M][ff] = silu(gate) * up; backward writes
 * d_gate_up [M][ld] from dh [M][ff]. */
int i2t_swiglu_fwd(void* stream, const void* gate_up, int ld, void* h, int M, int ff);
int i2t_swiglu_bwd(void* stream, const void* dh, const void* gate_up, int ld, void* d_gate_up, int M, int ff);

/* LoRA adapters (reference models/utils.py:46-65 -> peft: y = base(x) + lora_B(lora_A(dropout(x))) * alpha / r).  The rank-r products
 * are i2t_gemm_bf16 calls (rank padded to 64 by zero rows), the input dropout is i2t_dropout_apply; this is the GELU derivative behind
 * an adapted mlp.c_proj, whose input gradient is the fp32 sum of the base and adapter paths: out (bf16) = dh (fp32) * gelu_tanh'(pre). */
int i2t_dgelu_mul(void* stream, const float* dh, const void* pre, void* out, long n);
/* ... and behind an exact (erf) GELU (transformers' Falcon MLP, nn.GELU()): out = dh * gelu_erf'(pre). */
int i2t_dgelu_erf_mul(void* stream, const float* dh, const void* pre, void* out, long n);
/* out (bf16) = gelu(pre (bf16)), tanh form or (erf != 0) exact: the activation behind a projection whose GEMM cannot apply it while
 * also writing the pre-activation (the fp8 classes of i2t_gemm_fp8). */
int i2t_gelu_fwd(void* stream, const void* pre, void* out, long n, int erf);
/* One pass over an adapted layer's input x bf16 [M][K]: xcat[m][0..K) = x[m] (xcat bf16 [M][ldc] is the K-concatenated operand
 * [x | u] of the layer's GEMM) and, when xd is not null, xd [M][K] = dropout(x) with the elementwise mask (key, thr, scale; index
 * m * K + k, the index space of i2t_dropout_apply) -- the adapter's input (peft's lora_dropout). */
int i2t_lora_stage(void* stream, const void* x, void* xcat, int ldc, void* xd, long M, int K, unsigned drop_key, unsigned drop_thr,
                   float drop_scale);

/* Grouped small GEMMs for AdvancedPositionalBiasMLP (reference models/layers.py:617-638, decoder.py:231-232: every position owns a
 * private MLP, so one layer of the module is one GEMM per position).  Group g = position; its rows are rows [seg[g], seg[g+1]) of
 * the row-major operands (position-major order; seg = device int[n_groups + 1]; max_rows = the largest group), its weights
 * W_g = B + (g + group0) * b_group_stride (bf16 [N][K]), bias b_g = bias + (g + group0) * bias_group_stride (f32 [N]).
 *   mode 0: C[rows][N] = act(A[rows][K] . W_g^T + b_g) (+ residual)   act = I2T_ACT_GELU keeps the pre-activation in aux_out (bf16)
 *   mode 1: C[rows][K] = (A[rows][N] . W_g) * gelu'(aux_in) (+ residual)          (act = I2T_ACT_DGELU, or none)
 *   mode 2: C_g[N][K] (+)= A_g[rows][N]^T . B_g[rows][K]   with C_g = C + (g + group0) * c_group_stride (f32; B = the layer input rows)
 * group_ptr (device int, modes 0 / 1 with n_groups = 1, seg null): every one of the max_rows rows uses group *group_ptr + group0
 * (the decode step under hipGraph replay).  N, K multiples of 32.
 * i2t_grouped_colsum: out[(g + group0) * out_group_stride + n] += sum over the rows of group g of X[row][n]  (bias gradients). */
int i2t_grouped_gemm(void* stream, int mode, const void* A, int lda, const void* B, int ldb, long b_group_stride, void* C, int ldc,
                     long c_group_stride, int c_is_f32, const float* bias, long bias_group_stride, int act, const void* aux_in,
                     void* aux_out, int ld_aux, const float* residual, int ldr, int accumulate, const int* seg, int n_groups,
                     int max_rows, const int* group_ptr, int group0, int N, int K);
int i2t_grouped_colsum(void* stream, const void* X, int ld, const int* seg, int n_groups, float* out, long out_group_stride,
                       int group0, int N);

/* hipGraph capture around any sequence of the calls above (replaces the Python loop of
 * vision_encoder_decoder.py:143-180 with one replayed launch per token) */
int i2t_graph_capture_begin(void* stream);
int i2t_graph_capture_end(void* stream, void** graph_exec_out);
int i2t_graph_launch(void* graph_exec, void* stream);
int i2t_graph_destroy(void* graph_exec);

/* ---------------------------------------------------------------------------------------------------------
 * PretrainedViT (reference models/encoder.py:56-127): torchvision ViT-B/16 backbone + three heads.  The backbone's blocks run on
 * i2t_gemm_bf16 (I2T_ACT_GELU_ERF), i2t_attention_* and i2t_layernorm_fwd_eps; these are the pieces around them (csrc/vit.hip).
 *   i2t_patchify: conv_proj (p x p, stride p; encoder.py:60 -> torchvision VisionTransformer._process_input) as a GEMM: images f32
 *     [B][C][H][W] -> out bf16 [B (H/p) (W/p)][C p p], column order (c, ky, kx) = the flattened conv weight's.
 *   i2t_vit_tokens: x f32 [B][T][d] = [class_token | proj rows of the image] + pos_embedding (T = P^2 + 1).
 *   i2t_l2norm_fwd / _bwd: F.normalize(p = 2, eps 1e-12) over the last dim of M rows (encoder.py:118-119); y f32 and / or bf16,
 *     inv_norm f32 [M] saved; bwd: dx (+)= (dy - y <y, dy>) inv_norm.
 *   i2t_transpose_last2: dst[b][c][r] = src[b][r][c] (the (e, s) <-> (s, e) exchange around the peer_proj_wt GEMM, encoder.py:116).
 *   i2t_peer_lookup_fwd / _bwd: PeerLookup.forward after its linear maps (models/layers.py:78-109), one workgroup per row:
 *     scores f32 [M nhead][2 nq] = [query_left | query_right] scores, inp_proj bf16 [M][nhead din], residual f32 [M][dout],
 *     emb_in bf16 [units][din], emb_out bf16 [units][dout] -> out f32 [M][dout]; saved per (row, head, j < topk): expert unit,
 *     (left, right) query-unit indices, softmax score, pre-GELU dot.  bwd: dscores f32 (PRE-ZEROED by the caller), dinp_proj
 *     bf16, expert-table gradients accumulated with fp32 atomics (null = frozen).
 *   i2t_gemm_f32: z[M][N] = x[M][K] . P[K][N], fp32 FMA (the LSH projections: bucket decisions must not see bf16 rounding).
 *   i2t_lsh_embed_fwd / _bwd: CompositeCosineVectorEmbedding per slot (models/layers.py:112-143,190-219): z f32 [B][n_cls nK n_proj]
 *     -> bucket = #(grid points < z) -> mean over projections of table rows, summed over the nK resolutions; table k of slot s =
 *     tables + s slot_stride + tab_off[k] (f32 [(nbins[k] + 1) n_proj][dout]); grid k = grids + grid_off[k]; rows int [B][n_cls][nK][n_proj]
 *     saved; bwd scatters dy / n_proj into the tables' gradients (atomics).
 *   i2t_l2norm_groups_fwd / _bwd: the same normalisation for G matrices of `rows` rows that sit apart in one arena (the CosineLinear
 *     weights of the learnable LSH head, models/layers.py:147-153): row r of group g = x + group_off[g] + r d (offsets in elements,
 *     multiples of 4); y f32 [(g, r)][d] and inv_norm [G rows] come out contiguous; bwd writes dx (+)= at the same offsets of `dx`.
 *   i2t_lsh_soft_fwd / _bwd: LearnableCosineVectorEmbedding.gaussian_kernel (models/layers.py:183-191, top_k None) per (image b, slot s,
 *     resolution k, projection j): a_i = exp(-(c - mean_i)^2 / (2 (2 / nb_k)^2)), z = a / max(||a||_2, 1e-12), fp32 arithmetic, any
 *     nb_k >= 1.  c f32 [B][n_cls nK n_proj]; mean of (s, k) = params + s slot_stride + mean_off[k] (f32 [n_proj][nb_k]); z bf16
 *     [n_cls B][Ktot], row s B + b, column col_off[k] + j nb_k + i (col_off int [nK + 1], col_off[nK] = Ktot): the A operand of
 *     i2t_grouped_gemm with group = slot; inv_norm f32 [B][n_cls nK n_proj] saved.  bwd: dz f32 [n_cls B][Ktot] -> dc f32 (c's layout;
 *     t_ws = workspace of the same size) and g_params (+)= the means' gradient at the means' offsets (null = frozen): a sum over the
 *     batch, chunks of it meeting in fp32 atomics -- ONE fixed-order sum per element in deterministic mode.
 * --------------------------------------------------------------------------------------------------------- */
int i2t_patchify(void* stream, const float* images, void* out, int B, int C, int H, int W, int p);
int i2t_vit_tokens(void* stream, const float* proj, const float* cls, const float* pos, float* x, int B, int T, int d);
int i2t_l2norm_fwd(void* stream, const float* x, float* y, void* y_bf16, float* inv_norm, int M, int d);
int i2t_l2norm_bwd(void* stream, const float* dy, const float* x, const float* inv_norm, float* dx, int accumulate, int M, int d);
int i2t_transpose_last2(void* stream, const float* src, float* dst, void* dst_bf16, long B, int R, int C);
int i2t_peer_lookup_fwd(void* stream, const float* scores, const void* inp_proj, const float* residual, const void* emb_in,
                        const void* emb_out, float* out, int* sv_unit, int* sv_lr, float* sv_score, float* sv_dot, int M, int nhead,
                        int nq, int topk, int din, int dout);
int i2t_peer_lookup_bwd(void* stream, const float* dout, const void* inp_proj, const void* emb_in, const void* emb_out,
                        const int* sv_unit, const int* sv_lr, const float* sv_score, const float* sv_dot, float* dscores,
                        void* dinp_proj, float* g_emb_in, float* g_emb_out, int M, int nhead, int nq, int topk, int din, int dout_w);
int i2t_gemm_f32(void* stream, const float* x, const float* P, float* z, int M, int N, int K);
int i2t_lsh_embed_fwd(void* stream, const float* z, const float* tables, long slot_stride, const long* tab_off, const int* nbins,
                      const float* grids, const int* grid_off, float* out, int* rows, int B, int n_cls, int nK, int n_proj, int dout);
int i2t_lsh_embed_bwd(void* stream, const float* dy, const int* rows, float* g_tables, long slot_stride, const long* tab_off, int B,
                      int n_cls, int nK, int n_proj, int dout);
int i2t_l2norm_groups_fwd(void* stream, const float* x, const long* group_off, float* y, float* inv_norm, int G, int rows, int d);
int i2t_l2norm_groups_bwd(void* stream, const float* dy, const float* x, const long* group_off, const float* inv_norm, float* dx,
                          int accumulate, int G, int rows, int d);
int i2t_lsh_soft_fwd(void* stream, const float* c, const float* params, long slot_stride, const long* mean_off, const int* nbins,
                     const int* col_off, void* z_bf16, float* inv_norm, int B, int n_cls, int nK, int n_proj, int Ktot);
int i2t_lsh_soft_bwd(void* stream, const float* dz, const float* c, const float* inv_norm, const float* params, float* g_params,
                     long slot_stride, const long* mean_off, const int* nbins, const int* col_off, float* dc, float* t_ws, int B,
                     int n_cls, int nK, int n_proj, int Ktot);

/* ---------------------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange (replaces accelerate's DDP wrap, reference trainer.py:108-114,173-174):
 * one RCCL communicator per process (one process per GPU), all-reduce of the flat fp32 gradient arena in place over xGMI.
 * RCCL is bound at run time (the copy torch already loaded, else librccl.so.1); i2t_comm_available() = 0 means none was found.
 *   i2t_comm_unique_id: rank 0 fills a 128-byte id, the caller ships it to the other ranks (any out-of-band channel)
 *   i2t_comm_init: collective over all ranks (current HIP device of the calling thread); *comm_out = opaque handle
 *   i2t_comm_allreduce: buf[count] fp32 <- sum (mean != 0: mean) over ranks, asynchronous on `stream`; bf16_staging non-null
 *     (count bf16 elements, count % 4 == 0): the values travel as bf16 (half the bytes, one extra rounding per element)
 *   i2t_workspace_bytes: *bytes_out = scratch bytes the named entry point needs for a problem (M, N, K); 0 = none
 * --------------------------------------------------------------------------------------------------------- */
int i2t_comm_available(void);
int i2t_comm_unique_id(void* id_out, int bytes);
int i2t_comm_init(const void* id, int world, int rank, void** comm_out);
int i2t_comm_allreduce(void* comm, void* stream, float* buf, long count, int mean, void* bf16_staging);
int i2t_comm_destroy(void* comm);
int i2t_workspace_bytes(const char* entry, long M, long N, long K, long* bytes_out);

/* Deterministic mode: every reduction of the gradient path that combines workgroup partials with fp32 atomics (dW split-K
 * slices, column sums, LayerNorm / RMSNorm gain gradients, the gradient normaliser's sum, embedding scatter-adds, convolution
 * weight gradients) runs in one fixed order instead (one K slice, one workgroup, or one launch per workgroup).  Slow; two backward
 * passes of the same step are then bit-equal.  Default: the environment variable I2T_DETERMINISTIC (unset / 0 = off). */
int i2t_set_deterministic(int on);
int i2t_deterministic(void);

/* ---------------------------------------------------------------------------------------------------------
 * fp8 (OCP e4m3) operand path for frozen weights (BASELINE.json configs[4]; csrc/fp8.hip): C = (A8 . B8^T) * sa[m] * sb[n]
 * (+ bias[n]) (act: I2T_ACT_NONE | I2T_ACT_GELU | I2T_ACT_GELU_ERF, forward-only: no pre-activation output) (+ residual f32) on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales and per-row fp32 scales, fp32
 * accumulate, C bf16 or f32.  Rows of both operands are K contiguous bytes, zero-padded to the leading dimension (% 16).
 *   i2t_quant_rows_fp8: x (bf16 or f32) [M][ld] -> out e4m3 [M][ld_out], scale[m] = amax(row m) / 448 (1 for a zero row)
 *   i2t_quant_cols_fp8: W bf16 [N][ld] -> out e4m3 [K][ld_out] = W^T with a scale per k: the operand of dx = dy . W
 * --------------------------------------------------------------------------------------------------------- */
int i2t_quant_rows_fp8(void* stream, const void* x, int x_is_f32, int ld, void* out, int ld_out, float* scale, int M, int K);
int i2t_quant_cols_fp8(void* stream, const void* w, int ld, void* out, int ld_out, float* scale, int N, int K);
/* Producers that emit the e4m3 operand of the next i2t_gemm_fp8 themselves (no bf16 copy, no quantisation pass): RMSNorm forward
 * (d <= 8192; rstd for i2t_rmsnorm_bwd may be null), SwiGLU forward (h [M][ff]) and backward ([d gate | d up] [M][2 ff]); ff <= 12288.
 * Rows zero-padded to ld8 (% 16); scale[m] = amax(row m) / 448 as i2t_quant_rows_fp8, taken from the fp32 values.  The last argument: an
 * optional contiguous bf16 copy of the same row ([M][d] / [M][ff] / [M][2 ff]) for consumers that are not fp8 GEMMs (LoRA's rank products). */
int i2t_rmsnorm_fwd_fp8(void* stream, const float* x, const float* w, void* y8, int ld8, float* scale, float* rstd, int M, int d, float eps,
                        void* y_bf16);
int i2t_swiglu_fwd_fp8(void* stream, const void* gate_up, int ld, void* h8, int ld8, float* scale, int M, int ff, void* h_bf16);
int i2t_swiglu_bwd_fp8(void* stream, const void* dh, const void* gate_up, int ld, void* dgu8, int ld8, float* scale, int M, int ff,
                       void* dgu_bf16);
int i2t_gemm_fp8(void* stream, const void* A8, int lda, const float* sa, const void* B8, int ldb, const float* sb, void* C, int ldc,
                 int c_is_f32, int M, int N, int K, const float* bias, int act, const float* residual, int ldr);

/* ---------------------------------------------------------------------------------------------------------
 * Image preprocessing (csrc/preprocess.hip; replaces the reference's per-image host chain ToTensor -> Resize((H, W)) -> Normalize,
 * trainer.py): B decoded uint8 images of different sizes -> out fp32 [B][3][H][W] in one launch and one pass over the source.
 *   out[b][k] = resize(u_b[..., k]) * a_k + b_k,  a_k = 1 / (255 std_k), b_k = -mean_k / std_k (formed by the caller in fp64)
 * resize = torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=antialias != 0) on the raw 0..255
 * values: tap ranges and weights in fp64, rounded once to fp32; fp32 sums (width, then height); one fma per element.
 *   data: packed bytes, 16-byte aligned; image b at byte offsets[b] as [h_b][w_b][c_b] rows, shapes int32 [B][3] = (h, w, c),
 *     c = 1 (gray: replicated to the three output channels) or 3; every image ends at least 16 bytes before data + data_bytes
 *     (rows are read with 16-byte loads aligned down)
 *   max_side: the largest h or w in shapes (it sizes the LDS row buffers), 1..16384; H, W: 1..16384
 * An image whose shape or offset breaks these bounds is not read; its outputs are NaN. */
int i2t_preprocess_images(void* stream, const void* data, long data_bytes, const int64_t* offsets, const int* shapes, int B, int max_side,
                          float* out, int H, int W, float a0, float a1, float a2, float b0, float b1, float b2, int antialias);
/* The same kernel body over R boxes of those images: output r resizes the box regions[r] of image src to H x W and
 * mirrors it when flip is 1; R need not be B, an image may be named any number of times, the source is uploaded once.
 *   regions: int32 [R][6] = (src, top, left, bh, bw, flip), rows [top, top + bh) and columns [left, left + bw) of image src,
 *     0 <= src < B, the box inside the image, bh, bw >= 1, flip 0 or 1
 *   out[r][k] = flip(resize(u_src[top : top + bh, left : left + bw, k])) * a_k + b_k: the axes run over the box (n = bw, bh), taps clamp
 *     at the box's edges and no pixel outside it contributes; the flip is taken on the OUTPUT -- column x holds what column
 *     W - 1 - x of the unflipped result holds, bit for bit.  With the full box and flip 0 this is i2t_preprocess_images, bit for bit.
 * Only the rows and the byte span of a row that a workgroup's taps cover are read.  A region that breaks these bounds, or names an
 * image that i2t_preprocess_images would not read, is not read; its outputs are NaN, the other regions are untouched. */
int i2t_preprocess_regions(void* stream, const void* data, long data_bytes, const int64_t* offsets, const int* shapes, int B, int max_side,
                           const int* regions, int R, float* out, int H, int W, float a0, float a1, float a2, float b0, float b1, float b2,
                           int antialias);

#ifdef __cplusplus
}
#endif
#endif /* I2T_H */
