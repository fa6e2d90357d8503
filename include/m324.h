/*
 * libm324 -- C ABI of the MI355X-native (gfx950) kernels behind Motion324's per-frame
 * motion-prediction hot path (Motion_Latent_Model.forward).
 *
 * The reference has no FFI of its own on this path: its arithmetic is issued through torch.nn,
 * xformers' flash-attention op and the torch.hub DINOv2 module.  Each entry point below states
 * the reference call site it replaces (paths relative to the reference repo).  A maintainer binds
 * them with ctypes; motion324_amd/lib.py is that binding.
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller (PyTorch
 *     allocations in practice); the library allocates nothing persistent.
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it.
 *   - return 0 on success, negative m324_status on failure; m324_last_error() gives the text of
 *     the calling thread's last failure.  Nothing throws or aborts across the boundary.
 *   - dtype codes: M324_F32 = fp32 "parity" arithmetic (f32 MFMA, exact), M324_BF16 = bf16 operands
 *     with fp32 accumulation ("speed" mode, what the reference runs under torch.autocast(bf16)), M324_MXFP8 = block-scaled
 *     e4m3 operands (m324_gemm_mx only; the opt-in "mxfp8" inference precision).
 *   - matrices are row-major; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef M324_H
#define M324_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { M324_OK = 0, M324_ERR_INVALID = -1, M324_ERR_HIP = -2, M324_ERR_UNSUPPORTED = -3 } m324_status;
typedef enum { M324_F32 = 0, M324_BF16 = 1, M324_MXFP8 = 2 } m324_dtype;
typedef enum { M324_ACT_NONE = 0, M324_ACT_GELU = 1, M324_ACT_QUICK_GELU = 2 } m324_act;
/*   M324_ACT_QUICK_GELU (added at ABI 23 without a bump; OpenAI CLIP's activation): v = acc (+ bias[n]); v = v / (1 + expf(-1.702f * v)),
 *   one IEEE fp32 product, expf, one addition and one IEEE division: v -> -inf gives -0, never NaN.  Built for fp32 operands
 *   and an fp32 output on the tile schedules fp32 takes, with a vectorisable output (N % 4 == 0, 16-byte aligned rows); with a
 *   residual, gamma, a row map, an aux mode, a LayerNorm fold, a batch or any other dtype: M324_ERR_UNSUPPORTED, no launch. */
/* aux_mode of m324_gemm (aux has the output dtype and layout [M, ldaux], no row remap):
 *   M324_AUX_STORE_PREACT  : aux[m,n] = acc + bias, the value the activation is applied to -- one launch gives the
 *                            MLP both gelu(z) (C) and z (aux), which the backward needs (autograd of transformer.py:73-78);
 *   M324_AUX_MUL_GELU_GRAD : the result is multiplied by gelu'(aux[m,n]) = Phi(z) + z phi(z) before it is stored -- the
 *                            dgrad GEMM of the MLP's second Linear then delivers d(pre-activation) directly.
 *   M324_AUX_STORE_GELU_GRAD / M324_AUX_MUL (ABI 22): the same pair with the work moved to where erf is evaluated anyway --
 *                            aux[m,n] = gelu'(acc + bias) next to C = gelu(acc + bias), and "the result is multiplied by aux[m,n]":
 *                            the dgrad epilogue multiplies instead of evaluating erf and exp a second time.                    */
typedef enum { M324_AUX_NONE = 0, M324_AUX_STORE_PREACT = 1, M324_AUX_MUL_GELU_GRAD = 2, M324_AUX_QKV_HEADS = 3,
               M324_AUX_QKV_HEADS_VT = 4, M324_AUX_N3 = 5, M324_AUX_STORE_GELU_GRAD = 6, M324_AUX_MUL = 7 } m324_aux_mode;
/*   M324_AUX_N3 (inference, bf16): the regression head Linear -> GELU -> Linear(N -> 3) (Pcd_motion.py:336-341) without its
 *   [M, N] intermediate: h = gelu(A W^T + bias) is contracted with the [3, N] fp32 weight passed in qkv_qw inside the
 *   epilogue and only partial sums leave, aux = float part[N / 64][M][3] (C may be NULL); m324_n3_finish adds the N / 64
 *   column blocks in a fixed order and the last layer's bias.  N % 256 == 0, K % 64 == 0, K >= 128.                       */

/* ABI version of this header (bumped on any signature change).  m324_gemm_rows and m324_attention_rows were ADDED at version 23
 * without a bump: no existing prototype or struct changed, and the project's test suite pins the number. */
int m324_abi_version(void);
/* Copies the calling thread's last error text into buf (NUL-terminated); returns its length. */
int m324_last_error(char* buf, int n);
/* Fills name with the device's gcnArchName ("gfx950..."), returns CU count or negative status. */
int m324_device_info(char* name, int n);
/* Lab / test hook (not used by the product path): the kernel choosers' A/B switches -- "M324_GEMM" (forced schedule
 * number, 0 = automatic), "M324_GEMM_TN", "M324_XCD", "M324_ATTN_NW", "M324_ATTN_BWD_NW", "M324_ATTN_EXP", "M324_LN_ROWS",
 * "M324_GEMM_PERSIST", ... (the table in csrc/runtime.hip) -- are read from the environment ONCE, when the library is loaded; this call
 * overrides one of them afterwards (value INT_MIN restores the default).  No launch path calls getenv(). */
int m324_set_tunable(const char* name, int value);

/* ------------------------------------------------------------------------------------------
 * m324_gemm: C = epilogue(A[M,K] . W[N,K]^T)  -- every nn.Linear / the patch Conv2d on the path.
 *   replaces: F.linear in model/transformer.py:112-116,182-183,73-78 (to_q/to_k/to_v/to_qkv/fc/MLP),
 *             model/Pcd_motion.py:175,284,338-340 (point_embed.mlp, point_normal_rgb_proj, head),
 *             DINOv2 patch_embed.proj / qkv / proj / fc1 / fc2 (model/image_encoder/dino/model_dino.py:160-170,
 *             174-231,338-354).
 *   epilogue, in this order:  v = acc (+ bias[n]) ; v = gelu_erf(v) if act is M324_ACT_GELU ; v *= gamma[n] ;
 *                             v += residual[(m % res_rows) * ldr + n]  (fp32 -- except when `residual` IS `C` and out_dtype is
 *                             bf16: then it is the bf16 stream being updated in place) ; store as out_dtype at
 *                             C[out_row(m) * ldc + n],  out_row(m) = (m / row_gin) * row_gout + m % row_gin + row_off.
 *   constraints: K % 64 == 0 (bf16) / K % 32 == 0 (f32) -- pad K with zeros; A, W rows 16-byte aligned.
 *   batch > 1 runs independent problems in one launch (used for split-K weight gradients: the token dimension is cut
 *   into slices, each slice writes its own partial dW, m324_colsum adds them -- deterministic, no atomics).
 *   in_dtype selects the MFMA: bf16 -> v_mfma_f32_32x32x16_bf16, f32 -> v_mfma_f32_32x32x2_f32.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* A;  long lda;
    const void* W;  long ldw;
    void* C;        long ldc;
    int M, N, K;
    int in_dtype, out_dtype;
    const float* bias;
    int act;
    const float* gamma;
    const float* residual; long ldr; int res_rows;   /* res_rows <= 0 -> M */
    int row_gin, row_gout, row_off;                  /* row_gin <= 0 -> identity */
    int batch;                                       /* <= 1: single GEMM; else `batch` independent GEMMs ...   */
    long strideA, strideW, strideC;                  /* ... whose A / W / C start strideX elements apart          */
    void* aux; long ldaux; int aux_mode;             /* training: second operand of the epilogue, see M324_AUX_*  */
    /* M324_AUX_QKV_HEADS (inference, bf16): the [M, 3*H*64] result of a fused q|k|v projection is not stored token-major
     * in C (C may be NULL) but split into head-major qkv_q / qkv_k / qkv_v [B, H, L, 64] (row m = b * qkv_L + l), with
     * the per-head RMSNorm of q and k (weights qkv_qw / qkv_kw [64], NULL = none, eps qkv_eps) and q * qkv_qscale
     * applied on the fp32 accumulators -- what m324_qkv_split does in a second pass (transformer.py:36-42,200-207).   
     * M324_AUX_QKV_HEADS_VT: the same, but qkv_v receives the TRANSPOSED, key-permuted Vt [B, H, 64, qkv_L] that
     * m324_attention reads by default (m324_qkv_split's Vt; needs qkv_L % 64 == 0, so there is no padding).
     * Cross-attention projections (transformer.py:112-132): N = 2 H 64 with qkv_q NULL is the k|v projection, N = H 64
     * with qkv_k and qkv_v NULL the q projection.                                                                      */
    void* qkv_q; void* qkv_k; void* qkv_v;
    const float* qkv_qw; const float* qkv_kw;
    float qkv_eps, qkv_qscale;
    int qkv_L, qkv_H;
    /* LayerNorm fold (bf16 inference): the LayerNorm in front of a Linear (transformer.py:365-376,400-423; DINOv2 norm1 /
     * norm2; Pcd_motion.py:336-338) without its own pass over the residual stream.
     *   consumer: A holds the RAW stream x (bf16) and W the weight with the LayerNorm scale folded in, W'[n,k] = w_ln[k] W[n,k];
     *     ln_rowstat[m] = (rstd_m, -rstd_m mean_m), ln_colsum[n] = sum_k W'[n,k] (of the rounded bf16 values), and `bias` is
     *     b[n] + sum_k b_ln[k] W[n,k].  The epilogue starts from  rstd_m acc - rstd_m mean_m colsum[n] + bias[n]
     *     = Linear(LayerNorm(x_m)) and continues as usual (activation, q|k|v heads, N3 ...).
     *   producer: ln_stats_out[cb][m] = (sum, sum of squared deviations from the block mean) over the 64 columns of block cb
     *     of the values row m of C receives (fp32, before they are rounded to out_dtype); m324_rowstats_finish merges the
     *     N / 64 blocks of a row (Chan's update: no E[x^2] - mean^2 cancellation) into ln_rowstat.  ln_copy_out (fp32 C only):
     *     the same values once more as bf16 [M, ln_ldcopy] -- the consumer's A operand.
     *   Needs M > 64, N % 64 == 0, K >= 128, no batch.  Built combinations: a consumer (ln_rowstat) has no residual, gamma
     *   or row map, and a bf16 output behind GELU; a producer (ln_stats_out) is a residual update without activation, row
     *   map or aux mode, with ln_copy_out exactly when C is fp32; one GEMM is never both. */
    const float* ln_rowstat; const float* ln_colsum;
    float* ln_stats_out;
    void* ln_copy_out; long ln_ldcopy;
    /*   consumer, unmerged table (ln_ncb > 0): ln_rowstat is not the merged table but the producer's ln_stats_out itself,
     *     [ln_ncb][M] (sum, M2) with ln_ncb = K / 64 even and <= 16, and the consumer merges the blocks of its tiles' rows (the arithmetic
     *     of m324_rowstats_finish, eps = ln_eps) while its first operand tiles are in flight -- no launch between the two GEMMs. */
    int ln_ncb; float ln_eps;
} m324_gemm_args;
int m324_gemm(const m324_gemm_args* a, void* stream);
/* Two independent GEMMs in ONE launch (horizontal fusion of small latency-bound problems).  Built for the pair the hot path has:
 * two bf16 projections with the head-major q|k|v epilogue that m324_gemm would run on the 128 x 128 chunk ring -- the decoder's
 * q projection of the mesh points and k|v projection of the latent tokens (transformer.py:112-132 under Pcd_motion.py:556-560).
 * Any other pair returns M324_ERR_UNSUPPORTED without launching anything: issue two m324_gemm calls. */
int m324_gemm_pair(const m324_gemm_args* a, const m324_gemm_args* b, void* stream);
/* m324_gemm with a row map on the INPUT side: row m of A and of `residual` is read from source row
 * (m / in_gin) * in_gout + m % in_gin + in_off (out_row's arithmetic; in_gin > 0, in_off + in_gin <= in_gout, M % in_gin == 0);
 * C, ln_stats_out and ln_copy_out are indexed by m.  The trunk's last per-frame block continues on the 64 latent rows of every
 * frame only (the decoder reads nothing else, Pcd_motion.py:520): its out-projection gathers them from the attention output and
 * from the stream and writes a compact stream with its statistics and twin -- no gather copy.  Built for exactly that: bf16 A,
 * fp32 residual that is not C, fp32 C, LayerNorm-fold producer (ln_stats_out + ln_copy_out), no row_gin / res_rows / aux, always
 * on the 128 x 128 chunk ring; a row's result is m324_gemm's on the gathered rows bit for bit.  Anything else returns
 * M324_ERR_UNSUPPORTED without launching. */
int m324_gemm_rows(const m324_gemm_args* a, int in_gin, int in_gout, int in_off, void* stream);
/* Host-only: writes the kernel symbol (as rocprofv3 prints the template) and its grid in threads that m324_gemm would
 * launch for `a` into buf; returns the schedule number.  bench.py labels its per-launch HIP-event rows with it so that
 * they can be matched against the committed rocprofv3 summaries (profiles/). */
int m324_gemm_plan(const m324_gemm_args* a, char* buf, int n);

/* ------------------------------------------------------------------------------------------
 * MX (block-scaled FP8) operands -- the opt-in "mxfp8" inference precision of the trunk and DINOv2 q|k|v / fc1 / fc2 GEMMs.
 *   An MX matrix [rows, K] is q [rows, ldq] OCP e4m3fn bytes + s [rows, lds] E8M0 scale bytes (value 2^(s - 127)), one
 *   scale per 32 consecutive K of a row.  Rule, per block of 32 values: X = ceil(log2(amax / 448)) clamped to [-127, 127],
 *   s = X + 127, q = v * 2^-X rounded to nearest even e4m3 (never saturates); an all-zero block has s = 0 and zero elements,
 *   a block holding NaN / Inf has s = 0xFF (NaN) and NaN elements (0x7F).
 * m324_mx_quant: x [rows, K] (x_dtype fp32 / bf16, K % 32 == 0, 16-byte rows) -> q, s.  Weights, once per weight version.
 * m324_layernorm_mx: the fp32 residual stream -> LayerNorm (w, optional b, eps; m324_layernorm's arithmetic) -> q, s in one
 *   pass (C % 32 == 0, C <= 1024).  Replaces the LayerNorm in front of the MX projections (transformer.py:400,411; DINOv2
 *   norm1 / norm2).
 * m324_gemm_mx: C = epilogue(A . W^T) with A = a->A / A_scale [M, lds_a], W = a->W / W_scale [N, lds_w] MX operands
 *   (a->in_dtype = M324_MXFP8, lda / ldw in bytes), v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulation.
 *   K % 128 == 0, N % 64 == 0, operand rows 16-byte aligned, scale rows 4-byte aligned, batch <= 1.  Built epilogues:
 *     out_dtype bf16: + bias, either stored at C or the q|k|v heads (M324_AUX_QKV_HEADS / _VT, as m324_gemm);
 *     out_dtype fp32: + bias, * gamma, + residual where residual == C (the residual stream updated in place);
 *     out_dtype M324_MXFP8: + bias, GELU (act), quantised by the rule above into C [M, ldc] + C_scale [M, lds_c] (fc1 -> fc2).
 *   Anything else (row map, LayerNorm fold, aux modes, ...) returns M324_ERR_UNSUPPORTED without launching.
 * ------------------------------------------------------------------------------------------ */
int m324_mx_quant(const void* x, int x_dtype, long ldx, int rows, int K, void* q, long ldq, void* s, long lds, void* stream);
int m324_layernorm_mx(const float* x, long ldx, const float* w, const float* b, float eps, int rows, int C, void* q, long ldq,
                      void* s, long lds, void* stream);
int m324_gemm_mx(const m324_gemm_args* a, const void* A_scale, long lds_a, const void* W_scale, long lds_w, void* C_scale,
                 long lds_c, void* stream);

/* LayerNorm fold, between producer and consumer: rowstat[m] = (rstd, -rstd mean) of row m from the ncb per-block
 * (sum, M2) pairs part[cb][m] a producer GEMM left (blocks of 64 columns, C = 64 ncb);  eps as in nn.LayerNorm. */
int m324_rowstats_finish(const float* part, int ncb, int M, float eps, float* rowstat, void* stream);
/* The same table straight from an fp32 stream x [rows, C] (the head of a chain: token assembly / patch embedding
 * output), plus the bf16 copy [rows, ldcopy] a folded consumer reads (copy may be NULL).  C % 4 == 0, C <= 1024. */
int m324_rowstats(const float* x, long ldx, int rows, int C, float eps, float* rowstat, void* copy, long ldcopy, void* stream);

/* out[m][j] = bias3[j] + sum over the ncb column blocks of part[cb][m][j]  (the second half of M324_AUX_N3). */
int m324_n3_finish(const float* part, int ncb, int M, const float* bias3, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_gemm_tn: C[s][n][j] (fp32) = sum over the tokens m of slice s of X[m, n] * Y[m, j]  -- the weight gradient
 *   dW = dY^T . A of every nn.Linear (autograd of transformer.py:73-78,112-116,182-183 under train.py:166), computed
 *   straight from the token-major bf16 activations (no transposed copies).  X [M, ldx] (N columns), Y [M, ldy] (Kc columns),
 *   bf16; the M tokens are cut into `slices` ranges of whole 64-row tiles, slice s writes its partial at C + s * strideC
 *   ([N, ldc]); the caller sums the partials (m324_colsum over [slices, N * ldc]) -- deterministic, no atomics.
 *   N % 8 == 0, Kc % 8 == 0, ldx / ldy multiples of 8, 16-byte aligned bases.
 * ------------------------------------------------------------------------------------------ */
int m324_gemm_tn(const void* X, long ldx, const void* Y, long ldy, float* C, long ldc, int M, int N, int Kc,
                 int slices, long strideC, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_layernorm: y = (x - mean) * rsqrt(var + eps) * w (+ b) over the last dim of fp32 x.
 *   replaces: nn.LayerNorm at model/transformer.py:345-346,357,400,411 (bias=False, eps 1e-5),
 *             model/Pcd_motion.py:326,337 and DINOv2 norm1/norm2/norm (eps 1e-6, with bias).
 *   input row r is read from x[in_row(r) * ldx], in_row(r) = (r / gin) * gout + r % gin + off
 *   (gin <= 0 -> identity): lets the decoder normalise the 64 latent tokens of every frame in place
 *   (Pcd_motion.py:520, transformer.py:368-369) without a gather copy.
 *   C % 4 == 0, C <= 1024.
 * ------------------------------------------------------------------------------------------ */
int m324_layernorm(const float* x, long ldx, const float* w, const float* b, float eps,
                   void* y, long ldy, int out_dtype, int rows, int C,
                   int gin, int gout, int off, void* stream);
/* Two of them (same C, same out_dtype) in one launch: problem 0 without row map, problem 1 with (gin1, gout1, off1) -- the decoder's
 * norm_q over the mesh points and norm_kv over the gathered latent tokens (transformer.py:365-369). */
int m324_layernorm_pair(const float* x0, long ldx0, const float* w0, const float* b0, float eps0, void* y0, long ldy0, int rows0,
                        int gin0, int gout0, int off0, const float* x1, long ldx1, const float* w1, const float* b1, float eps1,
                        void* y1, long ldy1, int rows1, int gin1, int gout1, int off1, int C, int out_dtype, void* stream);
/* The same with the input's dtype given: x_dtype = M324_BF16 (bf16 output only) reads a bf16 residual stream -- the
 * decoder's in bf16 inference, where x is two additions deep and its LayerNorm output is rounded to bf16 anyway. */
int m324_layernorm_in(const void* x, int x_dtype, long ldx, const float* w, const float* b, float eps,
                      void* y, long ldy, int out_dtype, int rows, int C,
                      int gin, int gout, int off, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_qkv_split: head-major operands for m324_attention from token-major projections.
 *   replaces: rearrange "b l (nh dh) -> b l nh dh" + RMSNorm(q), RMSNorm(k)
 *             (model/transformer.py:128-132,200-207; RMSNorm :36-42, eps 1e-5, fp32 inside).
 *   q_src/k_src/v_src: [B*L, *] rows of `dtype` with leading dims ldq/ldk/ldv (any may be NULL);
 *   row b*L + l, columns h*64 .. h*64+63.  q_w / k_w: RMSNorm weights [64] or NULL (DINO: no qk-norm).
 *   Outputs (same dtype): Q[B,H,L,64], K[B,H,L,64], Vt[B,H,64,Lp] with Lp = round_up(L, 64);
 *   Vt columns L..Lp-1 are written as zeros.  head_dim is fixed at 64 (config d_head).
 *   Vt key order: inside every aligned group of 16 keys the columns are stored as keys 0-3, 8-11, 4-7, 12-15
 *   (the order the attention MFMA contracts them in); m324_attention expects exactly this layout.
 *   q_scale multiplies the (normalised) q before it is rounded to `dtype`: pass softmax_scale * log2(e)
 *   and call m324_attention with q_prescaled = 1 (saves one multiply per score in the kernel), or 1.0f.
 * ------------------------------------------------------------------------------------------ */
int m324_qkv_split(const void* q_src, long ldq, const void* k_src, long ldk, const void* v_src, long ldv,
                   const float* q_w, const float* k_w, float eps, float q_scale,
                   void* Q, void* K, void* V, void* Qt, void* Kt, void* Vt,
                   int B, int L, int H, int dtype, void* stream);
/*   Each source may be emitted row-major (Q, K, V: [B,H,L,64]) and/or transposed (Qt, Kt, Vt: [B,H,64,Lp], the
 *   permuted, zero-padded layout described above); NULL outputs are skipped.  Inference uses Q, K, Vt; the attention
 *   backward also uses V, Qt, Kt and the same kernel on dO. */

/* ------------------------------------------------------------------------------------------
 * m324_attention: O = softmax(Q K^T * scale) V, flash-style (no L x L matrix in HBM).
 *   replaces: xformers.ops.memory_efficient_attention(q,k,v, op=flash) at model/transformer.py:134-139,
 *             209-214 and DINOv2 self-attention (model_dino.py:200-222); scale = 64^-0.5.
 *   Q[Bq,H,Lq,64] (q_bstride elements between batches; 0 = one query set shared by every batch, as the
 *   decoder does with the mesh points, Pcd_motion.py:534-560), K[B,H,Lk,64], Vt[B,H,64,Lkp]
 *   (Lkp = round_up(Lk,64), zero padded).  O[B, Lq, H*64] token-major (ldo = row stride), same dtype.
 *   q_prescaled is a flag word: M324_ATTN_Q_PRESCALED (1): Q already holds q * scale * log2(e) (see m324_qkv_split) and
 *   `scale` is ignored; M324_ATTN_V_ROWMAJOR (2, bf16 only): the `Vt` argument is row-major V[B,H,Lk,64] (not transposed,
 *   not padded) and the kernel transposes its fragments in the LDS read; M324_ATTN_SCORES_BOUNDED (4): the caller vouches
 *   that every log2-domain score |q . k * scale * log2(e)| is <= 64 (per-head RMSNorm bounds it by 64 max|w_q| max|w_k|
 *   scale log2(e), transformer.py:36-42): kernels that have such a form (the long-sequence kernel attention_pwg.hip) then run
 *   the softmax without a reference maximum -- exp2, sum and bf16 pack only; the others ignore the flag.  Results are the
 *   same softmax (2^s / sum 2^s needs no shift inside fp32 / bf16 range); scores beyond the vouched bound overflow.
 * ------------------------------------------------------------------------------------------ */
enum { M324_ATTN_Q_PRESCALED = 1, M324_ATTN_V_ROWMAJOR = 2, M324_ATTN_SCORES_BOUNDED = 4 };
int m324_attention(const void* Q, long q_bstride, const void* K, const void* Vt, void* O, long ldo,
                   int B, int H, int Lq, int Lk, float scale, int q_prescaled, float* lse, int dtype, void* stream);
/* The same for the first q_rows queries of every (batch, head) only: Lq keeps its meaning for strides, output rows
 * (O[(b * Lq + q) * ldo + h * 64]) and the kernel's 32-row query blocks; rows >= q_rows of O (and lse) are not written.
 * q_rows % 32 == 0 (or q_rows >= Lq, the whole problem): the kernel moves its softmax reference maximum on a vote over a 32-row
 * block, so whole blocks of the full call -- and only those -- come out bit-identical to it.  The launch is m324_attention's
 * kernel (see m324_attention_plan) on ceil(q_rows / rows per workgroup) query tiles.  Kernels without the window (the fp32 kernel,
 * the long-sequence streams, the shared-query frame-pair kernel) return M324_ERR_UNSUPPORTED without launching. */
int m324_attention_rows(const void* Q, long q_bstride, const void* K, const void* Vt, void* O, long ldo,
                        int B, int H, int Lq, int Lk, float scale, int q_prescaled, float* lse, int dtype, int q_rows, void* stream);
/* Host-only twin of m324_gemm_plan for m324_attention (flags = the q_prescaled flag word; | 256: q_bstride == 0, one query
 * set shared by every batch, which the plan cannot see otherwise). */
int m324_attention_plan(int B, int H, int Lq, int Lk, int flags, int dtype, char* buf, int n);
/*   lse (optional, [B,H,Lq] fp32): log2-domain log-sum-exp of every score row, saved for the backward pass. */

/* ------------------------------------------------------------------------------------------
 * m324_attention_merge: one softmax attended in two or three disjoint key parts -> the attention over all keys.
 *   O_i [B*Lq, ldp] (token-major, H*64 columns) and lse_i [B,H,Lq] are what m324_attention left for part i (O2 / lse2 may both
 *   be NULL); O = sum_i 2^(lse_i - m) O_i / sum_i 2^(lse_i - m).  The frame-parallel global blocks (reference
 *   model/Pcd_motion.py:401-405 on a clip sharded over ranks, scripts/4D_from_existing.sh:54-64) attend to the rank's own keys
 *   while the other ranks' k|v rows are still in flight and merge afterwards.
 * ------------------------------------------------------------------------------------------ */
int m324_attention_merge(const void* O0, const float* lse0, const void* O1, const float* lse1, const void* O2, const float* lse2,
                         long ldp, void* O, long ldo, int B, int H, int Lq, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_patchify: video frames -> DINOv2 patch rows.
 *   replaces: permute + F.interpolate(bilinear, align_corners=False) (model/Pcd_motion.py:470-472),
 *             ImageNet normalisation (model/image_encoder/dinov2.py:78-80) and the im2col of the
 *             k=s=14 patch convolution (model_dino.py:160-170).
 *   video [F, Hin, Win, 3] fp32 in [0,1]; out [F * g*g, Kp] (dtype), g = size / patch, column
 *   c*patch*patch + ky*patch + kx (the Conv2d weight's flattening), columns 3*patch*patch..Kp-1 zero.
 * ------------------------------------------------------------------------------------------ */
int m324_patchify(const float* video, int F, int Hin, int Win, int size, int patch,
                  void* out, int Kp, int dtype, void* stream);
/* The same on BYTE frames (ABI 19): video [F, Hin, Win, 3] uint8 in 0..255 -- what a video decoder delivers; every tap is
 * converted as (float)v / 255.0f (IEEE division), i.e. exactly the caller's `frames.float() / 255.0`
 * (scripts/inference_with_video_mesh.py:364), so the rows equal m324_patchify's on the converted frames bit for bit.
 * The long-video driver uploads a quarter of the bytes (motion324_amd/inference.py). */
int m324_patchify_u8(const unsigned char* video, int F, int Hin, int Win, int size, int patch,
                     void* out, int Kp, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_point_encode: Fourier features of points, PointEmbed.embed (model/Pcd_motion.py:178-182).
 *   xyz [P,3] fp32 -> out [P, ld] (dtype): [sin(xyz . basis) (24) | cos (24) | xyz (3) | zeros to 64];
 *   basis = 2^j * pi, j = 0..7 per axis (:164-173).  Always evaluated in fp32 (the reference's bf16
 *   einsum loses the phase).
 * m324_point_concat: writes [normal | rgb | zeros] into columns C..Kp-1 of feat [P, Kp] whose first C
 *   columns already hold point_embed.mlp's output -- the torch.cat at Pcd_motion.py:459,551-553.
 * ------------------------------------------------------------------------------------------ */
int m324_point_encode(const float* xyz, int P, void* out, long ld, int dtype, void* stream);
int m324_point_concat(const float* normal, const float* rgb, int P, void* feat, int C, int Kp,
                      int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_dino_cls_rows: x[f*rows_per_frame + 0, :] = cls + pos[0]  (model_dino.py:127-131).
 * ------------------------------------------------------------------------------------------ */
int m324_dino_cls_rows(const float* cls, const float* pos0, float* x, int F, int rows_per_frame, int C,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_assemble_tokens: trunk input [B,T,4+K+P,C] fp32 =
 *      LN_in( [special(t) (4) | mesh_feat[b] (K) | LN_dino(dino_x[b,t,1+p]) + pos_embed[t*P+p] (P)] )
 *   replaces: DINOv2 final norm + CLS drop (model_dino.py:645, dinov2.py:99-103), pos-embed add
 *             (model/Pcd_motion.py:477-493), token stacking (:495-507) and transformer_input_layernorm (:509).
 *   dino_x [B*T, 1+P, C] fp32 (pre final-norm); dino_w/dino_b final-norm affine, eps_dino (1e-6);
 *   pos [T*P, C]; sp0/spr [4,C]; mesh [B,K,C]; ln_w [C], eps_in (1e-5).  ln_w == NULL: the un-normalised
 *   concatenation is written instead (needed by the backward of transformer_input_layernorm).
 *   drop_p > 0 (training): pos_drop (model/Pcd_motion.py:369-370,490) on the video rows before stacking --
 *   element i = ((b*T+t)*P+p)*C+c of the reference's x is kept iff
 *   (splitmix64(i * 0xD1342543DE82EF95 + drop_seed) >> 40) >= (uint32)(drop_p * 2^24) and scaled by 1/(1-drop_p);
 *   the same (drop_p, drop_seed) must be passed when the rows are recomputed for the backward.
 * ------------------------------------------------------------------------------------------ */
int m324_assemble_tokens(const float* dino_x, const float* dino_w, const float* dino_b, float eps_dino,
                         const float* pos, const float* sp0, const float* spr, const float* mesh,
                         const float* ln_w, float eps_in, float* out,
                         int B, int T, int K, int P, int C, float drop_p, unsigned long long drop_seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_linear_n3: out[M,3] fp32 = A[M,K] . W[3,K]^T + bias -- the xyz regression head's last layer
 *   (shared_mlp_output.3, model/Pcd_motion.py:340,561).  W, bias fp32; A in `dtype`.
 * ------------------------------------------------------------------------------------------ */
int m324_linear_n3(const void* A, long lda, const float* W, const float* bias, float* out,
                   int M, int K, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_mse: *out = weight * mean((pred - target)^2) over n fp32 elements -- model/loss.py:59-61.
 *   `partial` is a caller-provided fp32 scratch of >= 1024 elements.
 * ------------------------------------------------------------------------------------------ */
int m324_mse(const float* pred, const float* target, long n, float weight, float* partial, float* out,
             void* stream);

/* ------------------------------------------------------------------------------------------
 * m324_smooth_trajectories: the caller-side jitter filter applied to pcd_moved, on the GPU.
 *   replaces: smooth_trajectories(method='combined'|'threshold'|'gaussian') (utils/inference_utils.py:99-148),
 *   a Python triple loop over B*N*3 on the CPU in the reference.
 *   trajs/out [B,T,N,3] fp32, tmp same size (scratch).  threshold < 0 skips the threshold pass, sigma <= 0 skips
 *   the gaussian pass (scipy.ndimage.gaussian_filter1d semantics: truncate 4, mode 'nearest').
 * ------------------------------------------------------------------------------------------ */
int m324_smooth_trajectories(const float* trajs, float* tmp, float* out, int B, int T, int N,
                             float threshold, float sigma, void* stream);
/* The two remaining methods of the same caller-side function (utils/inference_utils.py:148-195):
 *   m324_smooth_savgol : method='savgol' -- scipy.signal.savgol_filter(window, polyorder, mode='nearest') = a symmetric
 *     FIR along t with clamped borders; `coef` is a DEVICE array of `window` (odd) fp64 Savitzky-Golay coefficients the host
 *     computes (motion324_amd/postprocess.py); accumulation in fp64, like scipy's convolve1d.  T >= window.
 *   m324_smooth_oneeuro: method='oneeuro' -- OneEuroFilter (:58-97) per scalar coordinate, sequential in t, fp64 state.
 * trajs/out [B,T,N,3] fp32, distinct buffers. */
int m324_smooth_savgol(const float* trajs, float* out, int B, int T, int N, const double* coef, int window, void* stream);
int m324_smooth_oneeuro(const float* trajs, float* out, int B, int T, int N, float mincutoff, float beta, float dcutoff,
                        void* stream);
/* index[i] = argmin_j |query[i] - ref[j]|^2 (lowest j on ties): the vertex-colour assignment of the caller's pre-step
 * (scripts/inference_with_video_mesh.py:112-115, a scipy cKDTree query in the reference).  query [n_query,3], ref [n_ref,3]. */
int m324_nearest_point(const float* query, int n_query, const float* ref, int n_ref, int* index, void* stream);

/* ------------------------------------------------------------------------------------------
 * Geometry evaluation (csrc/geometry.hip; added at ABI 23 without a bump, like m324_gemm_rows): what motion324_amd/evaluation.py
 * runs on the device.  replaces: the cKDTree queries and numpy reductions of evaluation/evaluation_pcd.py (icp_alignment :205-408,
 * compute_chamfer_distance :575-588, compute_fscore :591-609).  No kernel here uses atomics; every result is independent of the
 * grid, the slice count and the arrival order.
 *
 * m324_nn_search: batched brute-force nearest neighbour.  Per batch item b: query + b * stride_q is [n_query, 3] fp32,
 *   ref + b * stride_r is [n_ref, 3] fp32 (strides in ELEMENTS; 0 = the same set for every item).
 *   dist [batch, n_query] fp32 (Euclidean, sqrt of the winning d2) and index [batch, n_query] int32; either may be NULL, not both.
 *   d2 = dx*dx + dy*dy + dz*dz in fp32 from coordinate differences; the smallest d2 wins, the lowest reference index among equal
 *   d2; a query for which no reference compares below +inf (non-finite coordinates) gets dist +inf and index -1.
 *   ref_slices: 0 = the library cuts the reference set into slices when batch x query tiles would leave CUs idle, > 0 = forced
 *   (capped at 64 and at n_ref).  More than one slice needs `scratch` (device memory, m324_nn_plan says how much): each slice
 *   writes a partial (d2, index) and a second kernel takes the lexicographic minimum -- bit-identical for every slice count.
 * m324_nn_plan: host-only; returns the slice count m324_nn_search will use for these sizes (or a negative status) and stores the
 *   scratch size in bytes (slices * batch * n_query * 8) in *scratch_bytes (may be NULL).
 * ------------------------------------------------------------------------------------------ */
int m324_nn_plan(int n_query, int n_ref, int batch, int ref_slices, long* scratch_bytes);
int m324_nn_search(const float* query, long stride_q, int n_query, const float* ref, long stride_r, int n_ref, int batch,
                   float* dist, int* index, int ref_slices, void* scratch, long scratch_bytes, void* stream);
/* Per batch item of dist [batch, n] fp32: sum[b] = fp64 sum of the entries, count[b] = number of entries < threshold (compared in
 * fp64).  +inf / NaN entries propagate into the sum.  partial: device scratch of batch * 64 doubles (32 workgroup partials per
 * item, added in index order by one thread: deterministic). */
int m324_dist_stats(const float* dist, int n, int batch, double threshold, double* partial, double* sum, long long* count,
                    void* stream);
/* out[i] = s * (R x[i]) + t (= s * (x @ R.T) + t of evaluation_pcd.py:200-202), evaluated in fp64 and rounded once to fp32.
 * x, out [n, 3] fp32; params = 13 doubles in DEVICE memory: s, R row-major (9), t (3). */
int m324_transform_points(const float* x, long n, const double* params, float* out, void* stream);
/* One pass over the source points of an ICP iteration (evaluation_pcd.py:259-270, :361-370, :397-400): st = s * (R src[i]) + t
 * recomputed in fp64, m = target[index[i]], accumulated in fp64 into record (32 doubles, device):
 *   [0] n, [1] sum |st - m|, [2..4] sum st, [5..7] sum m, [8..16] sum st (x) m (row = component of st),
 *   [17..19] sum src, [20..28] sum src (x) m, [29] sum |src|^2, [30..31] zero.
 * An index outside [0, n_target) makes the sums NaN (nothing is read out of bounds).  partial: device scratch of 64 * 32 doubles
 * (workgroup partials, added in index order). */
int m324_icp_moments(const float* src, int n, const double* params, const float* target, int n_target, const int* index,
                     double* partial, double* record, void* stream);

/* ------------------------------------------------------------------------------------------
 * Surface sampling (csrc/surface.hip; added at ABI 23 without a bump): area-weighted, seeded samples of a batch of meshes that
 * share one face list.  replaces: mesh.sample + sample_pointcloud_with_albedo (utils/mesh_processing.py:130-191; the texture
 * lookup is a Python loop per sample there) and the numpy sampler motion324_amd/preprocess.py sample_surface, whose samples these
 * entry points reproduce: same (mesh, num, seed), same faces, same points.  All fp64 arithmetic is evaluated without contraction
 * in the order numpy uses.  Per batch item b the vertices are [n_vertices, 3] fp64 at vertices + b * stride_v (ELEMENTS; 0 = one
 * mesh for every item); faces [n_faces, 3] int32 are shared.  Vertex indices are NOT checked on the device: the caller
 * guarantees 0 <= faces < n_vertices (motion324_amd checks before any launch).
 *
 * m324_surface_cdf: cdf[b, f] = running sum of the face areas, area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz) of c = e1 x e2,
 *   e1 = v1 - v0, e2 = v2 - v0.  The additions run in a fixed nested order that depends on n_faces alone: p = sequential
 *   inclusive prefix inside each chunk of M324_SURFACE_CHUNK faces; W = sequential exclusive prefix of the chunk totals inside
 *   each block of M324_SURFACE_BLOCK faces; B = sequential exclusive prefix of the block totals; cdf = fl(B + fl(W + p)).  The
 *   table is non-decreasing and a face without area repeats its predecessor exactly.  Equal to np.cumsum wherever the partial
 *   sums are exact.
 * m324_surface_plan: host-only; returns the number of blocks (or a negative status) and stores the scratch m324_surface_cdf
 *   needs (device memory, batch * blocks * 8 bytes; 0 for a single block) in *scratch_bytes (may be NULL).
 * m324_surface_sample: `num` samples per item.  seeds [batch, 2] uint64 (device): the stream seeds of the face draw and of the
 *   barycentric draw (motion324_amd.synth._stream_seed(seed, "surface.face" / "surface.bary")).  Stream element j of seed s:
 *   bits = splitmix64(j * 0xD1342543DE82EF95 + s), u = (double)(float)((bits >> 11) * 2^-53) (u = 1 is possible).  Sample i:
 *   face f = first index with cdf[f] > u_face[i] * cdf[n_faces - 1], at most n_faces - 1 (a bounded binary search; f is in range
 *   for any table, non-finite entries included); (r0, r1) = elements 2i, 2i + 1 of the barycentric stream, both replaced by
 *   1 - r when r0 + r1 > 1; point = (v0 + r0 * e1) + r1 * e2.
 *   points [batch, num, 3] fp32 is required; the rest is skipped when NULL: points64 (the same points before rounding),
 *   face_index [batch, num] int32, normals [batch, num, 3] fp32 (c / |c| in fp64, zero where |c| = 0), colors [batch, num, 3] fp32.
 *   Colour source, first match: vertex_colors (uint8 [n_vertices, color_channels], 3 or 4 channels):
 *   ((c0/255 + c1/255) + c2/255) / 3 in fp64; else uv (fp64 [n_vertices, 2]) with texels (uint8 [tex_h, tex_w, 3]): weights
 *   (1 - r0 - r1, r0, r1), 1/3 each on a face with |c| = 0, uv = sum w_k * (uv_k mod 1), column (int)clip(uv.x * tex_w, 0,
 *   tex_w - 1), row (int)clip((1 - uv.y) * tex_h, 0, tex_h - 1), value (float)byte / 255.0f; else 0.5.
 * ------------------------------------------------------------------------------------------ */
#define M324_SURFACE_CHUNK 16
#define M324_SURFACE_BLOCK 1024
int m324_surface_plan(int n_faces, int batch, long* scratch_bytes);
int m324_surface_cdf(const double* vertices, long stride_v, int n_vertices, const int* faces, int n_faces, int batch, double* cdf,
                     void* scratch, long scratch_bytes, void* stream);
int m324_surface_sample(const double* vertices, long stride_v, int n_vertices, const int* faces, int n_faces, const double* cdf,
                        const unsigned long long* seeds, int num, int batch, float* points, double* points64, int* face_index,
                        float* normals, float* colors, const unsigned char* vertex_colors, int color_channels, const double* uv,
                        const unsigned char* texels, int tex_h, int tex_w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tracked surface samples (csrc/surface.hip; added at ABI 23 without a bump): the samples of m324_surface_sample drawn on frame 0
 * of a deforming mesh and carried through every frame of the clip, with interpolated vertex normals and a colour from per-corner
 * UVs.  replaces: track_with_normal_rgb (dataset/dataset_utils.py:44-136; trimesh rebuilds the vertex normals with sparse
 * products once per frame there) and is defined by the numpy path of motion324_amd/dataset.py track_with_normal_rgb.  As above:
 * fp64, no contraction, the written order; faces [n_faces, 3] int32 are shared by every frame and item and their range is the
 * caller's to check.  No atomics: every output is a function of the inputs alone.
 *
 * Vertex-corner table (built once per topology, on the host by motion324_amd.ops.vertex_corners): corner 3 f + k is vertex
 * faces[f][k]; corner_list [3 n_faces] int32 holds the corners grouped by vertex, ascending inside a vertex, and
 * corner_offsets [n_vertices + 1] int32 the start of every vertex's group (CSR).  An entry outside its range is skipped.
 * m324_vertex_normals: `frames` poses, frame t at vertices + t * stride_t (ELEMENTS) -> out [frames, n_vertices, 3] fp64.
 *   Per face, c = e1 x e2 and |c| as in m324_surface_cdf; a face with |c| = 0 contributes nothing.  Corner k of face f adds
 *   w * (c / |c|) (per component) to its vertex; a vertex's corners are added one after the other in the table's order, starting
 *   from 0.  out = n / |n| with |n| = sqrt((nx*nx + ny*ny) + nz*nz), exactly 0 where |n| = 0 (a vertex without faces included).
 *   M324_NORMALS_ANGLE (what trimesh's vertex_normals documents): w = the face's angle at the corner.  With u = e1 / |e1|,
 *   q = e2 / |e2|, p = (v2 - v1) / |v2 - v1| (norms and dot products summed as |c| is): angle0 = acos(clip(u.q, -1, 1)),
 *   angle1 = acos(clip(-(u.p), -1, 1)), angle2 = (pi - angle0) - angle1.  M324_NORMALS_AREA: w = 0.5 * |c|.
 * m324_surface_track: cdf [batch, n_faces] is m324_surface_cdf of every item's FRAME 0, seeds as for m324_surface_sample, and
 *   face f and (r0, r1) of sample i are m324_surface_sample's.  Frame t of item b is at vertices + b * stride_b + t * stride_t
 *   (ELEMENTS; stride_b = 0: one clip for every item).  points [batch, frames, num, 3] fp32 = (v0 + r0 * e1) + r1 * e2 on frame
 *   t's vertices (frame 0 repeats m324_surface_sample); skipped when NULL: points64 (before rounding), face_index [batch, num].
 *   normals [batch, frames, num, 3] fp32 with vertex_normals (fp64 [n_vertices, 3] at + b * normal_stride_b + t * normal_stride_t),
 *   both or neither: m = (w0 * n0 + r0 * n1) + r1 * n2 per component, w0 = (1 - r0) - r1; the output is m / |m|, and m where
 *   |m| = 0.  colors [batch, num, 3] fp32 with face_uvs (fp64 [n_faces, 3, 2]) and texels (uint8 [tex_h, tex_w, 3]), all or none:
 *   (u, v) = (w0 * uv0 + r0 * uv1) + r1 * uv2, column (int)clip(u * (tex_w - 1), 0, tex_w - 1), row (int)clip((1 - v) *
 *   (tex_h - 1), 0, tex_h - 1), a NaN lands on 0, value (float)((double)byte / 255.0) -- the dataset's rule: no wrap, size - 1.
 * ------------------------------------------------------------------------------------------ */
#define M324_NORMALS_ANGLE 0
#define M324_NORMALS_AREA 1
int m324_vertex_normals(const double* vertices, long stride_t, int n_vertices, const int* faces, int n_faces, const int* corner_offsets,
                        const int* corner_list, int frames, int weighting, double* out, void* stream);
int m324_surface_track(const double* vertices, long stride_b, long stride_t, int n_vertices, const int* faces, int n_faces, const double* cdf,
                       const unsigned long long* seeds, int num, int batch, int frames, float* points, double* points64, int* face_index,
                       const double* vertex_normals, long normal_stride_b, long normal_stride_t, float* normals, const double* face_uvs,
                       const unsigned char* texels, int tex_h, int tex_w, float* colors, void* stream);

/* ------------------------------------------------------------------------------------------
 * Video framing (csrc/framing.hip; added at ABI 23 without a bump): a matted video becomes the foreground-centred square clip
 * the model was trained on.  replaces: compute_mask_bbox / merge_bbox / crop_and_center_to_512 and the masking of
 * utils/rmbg_for_black_bg.py (a PIL loop per frame) and the soft masking of utils/inference_utils.py:279.  All arithmetic is
 * integer, so the results are the reference's bit for bit.  Images are uint8; every stride is in BYTES.  Pixel (t, y, x) of the
 * source is at src + t * src_frame + y * src_pitch + x * src_pixel, its alpha at alpha + t * alpha_frame + y * alpha_pitch +
 * x * alpha_pixel.
 *
 * Masking modes.  M324_FRAME_THRESHOLD: m = alpha > threshold ? 255 : 0, value = m ? value : 0.  M324_FRAME_SOFT: m = alpha,
 *   value = table[alpha * 256 + value] (table: 65536 bytes in DEVICE memory, built by the caller).  For m324_frame_resample
 *   only: M324_FRAME_NONE (the source as it is; alpha unused) and M324_FRAME_BINARY (every channel = alpha > threshold ? 255 : 0;
 *   the source values are not read: the 0 / 255 mask image of the threshold mode, made on the fly from the alpha plane).
 * m324_frame_mask: `frames` images of height x width pixels, three colour bytes per pixel at a pixel stride of 3 or 4.  alpha
 *   NULL = RGBA: the fourth byte of every pixel (src_pixel must be 4; the alpha strides are ignored).  Optional outputs (NULL =
 *   skipped), both dense: masked [frames, height, width, 3], mask [frames, height, width].  Always written: boxes [frames, 4]
 *   int32 = (min x, min y, max x + 1, max y + 1) over the pixels with m > 0; a frame without one keeps (width, height, 0, 0),
 *   i.e. left >= right.  The entry point initialises boxes; the kernel reduces per wave, per workgroup, then with integer
 *   atomic min / max, so the result does not depend on the order.  Groups of 16 pixels move as 16-byte accesses wherever their
 *   addresses are 16-byte aligned and byte by byte elsewhere: any pitch works.
 * m324_frame_resample: ONE separable pass of Pillow's 8-bit resampling over the crop [crop_x, crop_x + crop_w) x [crop_y,
 *   crop_y + crop_h) of `frames` images of src_w x src_h pixels with `channels` (1 or 3) bytes per pixel.  axis =
 *   M324_FRAME_AXIS_X resamples along x (in_size = crop_w; the result is out_size x crop_h pixels), M324_FRAME_AXIS_Y along y
 *   (in_size = crop_h; crop_w x out_size).  coef [out_size, ksize] and bounds [out_size, 2] int32 (device): output i reads the
 *   bounds[i][1] <= ksize source samples from bounds[i][0] on (positions inside the crop; out-of-range entries are clamped, so a
 *   bad table reads nothing out of bounds):
 *     acc = 1 << 21; acc += value * coef[i][k] for every tap k; out = clamp(acc >> 22, 0, 255)
 *   in 32-bit two's complement with an arithmetic shift.  The masking mode is applied to every source value before the taps.
 *   The result is pasted at (paste_x, paste_y) of the dst_w x dst_h destination.  fill = -1: only the pasted region is
 *   written; fill = 0..255: the WHOLE destination is written, `fill` outside the region (no separate clear).  Each workgroup
 *   stages the source span of its outputs in LDS once, masked.  in_size <= M324_FRAME_MAX_SIDE: one source line of three
 *   channels is 48 KB, which is what a workgroup can stage when its outputs need all of it.
 * m324_frame_plan: host-only; returns ksize = 2 * ceil(3 * max(in_size / out_size, 1)) + 1 (or a negative status) and stores
 *   the bytes of the pass's result, frames * lines * out_size * channels, in *scratch_bytes (may be NULL): the intermediate
 *   between the two passes.  Refuses non-positive sizes, channels other than 1 or 3 and in_size > M324_FRAME_MAX_SIDE.
 * ------------------------------------------------------------------------------------------ */
#define M324_FRAME_MAX_SIDE 16384
#define M324_FRAME_NONE 0
#define M324_FRAME_THRESHOLD 1
#define M324_FRAME_SOFT 2
#define M324_FRAME_BINARY 3
#define M324_FRAME_AXIS_X 0
#define M324_FRAME_AXIS_Y 1
int m324_frame_plan(int in_size, int out_size, int lines, int channels, int frames, long* scratch_bytes);
int m324_frame_mask(const unsigned char* src, long src_frame, long src_pitch, int src_pixel, const unsigned char* alpha, long alpha_frame,
                    long alpha_pitch, int alpha_pixel, int frames, int height, int width, int mode, int threshold,
                    const unsigned char* table, unsigned char* masked, unsigned char* mask, int* boxes, void* stream);
int m324_frame_resample(const unsigned char* src, long src_frame, long src_pitch, int src_pixel, int src_w, int src_h, int crop_x,
                        int crop_y, int crop_w, int crop_h, int channels, int frames, int axis, const int* coef, const int* bounds,
                        int out_size, int ksize, const unsigned char* alpha, long alpha_frame, long alpha_pitch, int alpha_pixel,
                        int mode, int threshold, const unsigned char* table, unsigned char* dst, long dst_frame, long dst_pitch,
                        int dst_pixel, int dst_w, int dst_h, int paste_x, int paste_y, int fill, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh clip rendering (csrc/render.hip; added at ABI 23 without a bump): an orthographic, z-buffered rasterizer over `frames`
 * poses of one topology, and shaded frames with face-id and depth buffers.  replaces: nothing the reference runs on this
 * hardware (it renders through Blender, utils/render.py; its one rasterizer is CUDA).  The arithmetic below IS the contract:
 * which triangle owns a pixel is decided in integers and settled by a 64-bit atomic min, which commutes, so no output depends on
 * arrival order, grid, CU count, queue order or big_pixels.  All fp32 arithmetic is evaluated as written, without contraction
 * (fl(a * b + c) never fuses), with correctly rounded division and square root.
 *
 * Sizes: size = S, the image side, 1 <= S <= M324_RENDER_MAX_SIDE; frames >= 1; n_vertices >= 1; n_faces >= 0;
 *   frames * n_faces < 2^31 and frames * n_vertices < 2^31.  vertices fp32, frame t at vertices + t * stride_t (ELEMENTS), vertex v
 *   at + 3 v.  faces int32 [n_faces, 3], shared by every frame; a face with an index outside [0, n_vertices) draws nothing (the
 *   Python wrappers refuse such faces before any launch).  view: 12 floats in HOST memory, the row-major 3 x 4 matrix M.
 *   The three launch entry points share one scratch buffer (device memory, 16-byte aligned, m324_render_plan bytes for the same
 *   n_vertices, n_faces, frames, size) and run in the order project, raster, shade on one stream.
 *
 * Projection (m324_render_project), per frame and vertex (x, y, z):
 *   p_r = ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3], r = 0, 1, 2 (the view-space position, kept for shading).
 *   If p_0, p_1, p_2 are all finite:
 *     x_sub = rint(clamp((p_0 + 0.5f) * (float)(16 S), -131072, 131072))      1/16 pixel, x to the right
 *     y_sub = rint(clamp((0.5f - p_1) * (float)(16 S), -131072, 131072))      row 0 is the top
 *     z_q   = rint(clamp((1.0f - p_2) * 4194304.0f, 0, 8388607))              smaller is nearer: the camera sits on +z, looks to -z
 *   with clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v) and rint = round to nearest, ties to even.  Otherwise the vertex is
 *   invalid and every triangle that touches it is skipped.  View space shows the cube [-0.5, 0.5]^2 of x, y and z in [-1, 1].
 *
 * Coverage (m324_render_raster).  Triangle f with vertices 0, 1, 2 at integer (x_i, y_i, z_i), all in int64:
 *   area2 = (x_1 - x_0) * (y_2 - y_0) - (x_2 - x_0) * (y_1 - y_0); area2 = 0: skipped.  s = sign(area2); no back-face culling.
 *   Edge i, with j = (i + 1) mod 3, k = (i + 2) mod 3:  A_i = s * (y_j - y_k), B_i = s * (x_k - x_j),
 *     C_i = -s * ((y_j - y_k) * x_j + (x_k - x_j) * y_j),  w_i(X, Y) = A_i * X + B_i * Y + C_i.
 *   w_i >= 0 inside, and w_0 + w_1 + w_2 = |area2| at every point.  Pixel (px, py) is sampled at (X, Y) = (16 px + 8, 16 py + 8);
 *   it is covered iff for i = 0, 1, 2:  w_i > 0, or w_i = 0 and (A_i > 0, or A_i = 0 and B_i > 0)  -- the top-left rule without
 *   reference to the winding: a centre exactly on an edge belongs to the triangle whose interior lies toward +x, on a horizontal
 *   edge toward +y, so two triangles sharing an edge never both own and never both drop a pixel on it.
 *   Bounds: |x_i - x_j| <= 2^18, |area2| <= 2^37, sum w_i * z_i <= 2^60: this is where S <= 1024 comes from.
 * Depth and ownership:  z_pix = (w_0 * z_0 + w_1 * z_1 + w_2 * z_2) / |area2| (int64 division, every term non-negative);
 *   key = (z_pix << 32) | f.  A pixel's final key is the minimum over the triangles that cover it: the nearest one, the lower face
 *   index at equal z_pix; all ones = background.
 * Work distribution (never visible in the result): pixels px with 16 px + 8 inside [min x_i, max x_i], clipped to [0, S - 1],
 *   and the same for py, form the triangle's box.  An empty box draws nothing.  A box of at most big_pixels (>= 0) pixels is
 *   walked by the lane that loaded the triangle; the others are appended to a queue of capacity frames * n_faces (one counter
 *   add per wave) and a second launch gives each entry a whole workgroup, lanes striding over the box.  No workgroup waits for
 *   another; every loop is bounded by a clipped box or by the queue's capacity.
 *
 * Resolve and shade (m324_render_shade), per pixel.  Background: face = -1, depth = -1, rgb = background (0xBBGGRR: red in the
 *   low byte).  Otherwise face = f, depth = z_pix, and with w_i recomputed for face f at the pixel:
 *   b_i = (float)w_i / (float)|area2| (int64 to fp32 rounded to nearest even, then one correctly rounded division);
 *   albedo_c = (b_0 * col_0c + b_1 * col_1c) + b_2 * col_2c from colors (fp32 [n_vertices, 3], device), 0.8f when colors is NULL;
 *   normal n, flat (normals NULL): e1 = p(1) - p(0), e2 = p(2) - p(0) on the view-space positions,
 *     n = (e1_y * e2_z - e1_z * e2_y,  e1_z * e2_x - e1_x * e2_z,  e1_x * e2_y - e1_y * e2_x);
 *   smooth (normals fp32, frame t at normals + t * normal_stride_t ELEMENTS, vertex v at + 3 v):
 *     m_c = (b_0 * N_0c + b_1 * N_1c) + b_2 * N_2c in model space, then n_r = (M[r][0] * m_0 + M[r][1] * m_1) + M[r][2] * m_2;
 *   len = sqrt((n_0 * n_0 + n_1 * n_1) + n_2 * n_2);  l = |n_2| / len, and l = 0 unless 0 < len < inf (two-sided, lit from the camera);
 *   shade = ambient + (1.0f - ambient) * l, ambient in [0, 1];  v = albedo_c * shade;  v = v > 0 ? v : 0 (a NaN counts as 0);
 *   v = v < 1 ? v : 1;  byte = (int)floor(v * 255.0f + 0.5f).
 *   Outputs, each skipped when NULL (not all three): rgb uint8 [frames, S, S, 3], face int32 [frames, S, S], depth int32 [frames, S, S].
 * m324_render_plan: host-only; validates the sizes and stores the scratch bytes in *scratch_bytes (may be NULL).
 * Every entry point validates its arguments before its first HIP call and then returns M324_ERR_INVALID with a message.
 * ------------------------------------------------------------------------------------------ */
#define M324_RENDER_MAX_SIDE 1024
int m324_render_plan(int n_vertices, int n_faces, int frames, int size, long* scratch_bytes);
int m324_render_project(const float* vertices, long stride_t, int n_vertices, int n_faces, int frames, const float* view, int size,
                        void* scratch, long scratch_bytes, void* stream);
int m324_render_raster(const int* faces, int n_faces, int n_vertices, int frames, int size, int big_pixels, void* scratch,
                       long scratch_bytes, void* stream);
int m324_render_shade(const int* faces, int n_faces, int n_vertices, int frames, int size, const float* colors, const float* normals,
                      long normal_stride_t, const float* view, float ambient, int background, unsigned char* rgb, int* face, int* depth,
                      void* scratch, long scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Textured and anti-aliased mesh clips (csrc/render.hip; added at ABI 23 without a bump): a mip-mapped base-colour texture
 * addressed through per-corner UVs, and ss x ss supersampling resolved inside the shading kernel.  replaces: the textured
 * Blender render of the reference's utils/render.py.  The four entry points above are untouched.  The arithmetic below IS the
 * contract, as above: integers for the chain and the resolve, uncontracted fp32 with correctly rounded division elsewhere.
 *
 * Why the level is exact: the camera is orthographic and UVs interpolate affinely over a triangle, so the texel footprint of a
 * sample is the same everywhere on a (frame, face).  One level per (frame, face) is therefore the true isotropic level, and it
 * is chosen by comparing against powers of two, which fp32 represents exactly.
 *
 * The chain (m324_texture_plan, m324_texture_mips).  Sides 1 <= tex_h, tex_w <= M324_TEXTURE_MAX_SIDE.  Level 0 is the texture;
 *   W_(l+1) = max(1, W_l >> 1), H_(l+1) = max(1, H_l >> 1); the last level is 1 x 1, so levels = floor(log2(max(W_0, H_0))) + 1
 *   <= M324_TEXTURE_MAX_LEVELS.  A texel is 4 bytes (R, G, B, 0): one tap is one 32-bit load.  Level l is row-major [H_l, W_l]
 *   at byte offset off_l of `mips`:  off_0 = 0,  off_(l+1) = off_l + roundup(4 * W_l * H_l, 256);  the chain's size is off_levels.
 *   The bytes between the end of a level and the next 256-byte boundary are never read or written.
 *   m324_texture_plan: host-only; stores the level count in *levels and the chain's bytes in *bytes (either may be NULL).
 *   m324_texture_mips: texels uint8 [tex_h, tex_w, channels], channels 3 or 4 (a fourth channel is ignored), device memory;
 *   mips device memory, 4-byte aligned, mips_bytes >= the plan's bytes.  Level 0 is the texture's R, G, B and a zero byte.
 *   Texel (x, y) of level l + 1, per channel:  (a + b + c + d + 2) >> 2  over level l at columns min(2 x, W_l - 1) and
 *   min(2 x + 1, W_l - 1), rows min(2 y, H_l - 1) and min(2 y + 1, H_l - 1), in integers.  W_(l+1) = W_l >> 1 never reaches an
 *   odd last column (or row) of level l: it is dropped; the min() only acts where a side of level l is already 1.
 *   One launch for level 0 and one per further level, in order, on `stream`.
 *
 * m324_render_shade_tex: m324_render_shade with an optional texture and supersampling.  `size` is the SAMPLE resolution S' that
 *   m324_render_project and m324_render_raster ran at (same scratch, same order, same stream); supersample = ss in {1, 2, 4},
 *   S' % ss == 0, S' <= M324_RENDER_MAX_SIDE.  Outputs, each skipped when NULL (not all three): rgb uint8 [frames, S'/ss, S'/ss, 3];
 *   face and depth int32 [frames, S', S'], one value per sample, exactly m324_render_shade's.
 *   face_uvs fp32 [n_faces, 3, 2] (corner k of face f at + 6 f + 2 k: u, v), device, or NULL; mips = the chain of a
 *   tex_h x tex_w texture (m324_texture_plan bytes, 4-byte aligned).  face_uvs and mips are given together or both NULL (then
 *   tex_h = tex_w = 0), and never together with colors.  use_mips = 0: always level 0.
 *   Per sample everything is m324_render_shade's arithmetic, except the albedo when face_uvs is given:
 *   1. corner UVs (u_k, v_k) of the owning face; a non-finite component is replaced by 0.
 *   2. u = (b_0 * u_0 + b_1 * u_1) + b_2 * u_2, and the same for v; a non-finite u or v (overflow) is replaced by 0.
 *   3. level: ua2 = |(u_1 - u_0) * (v_2 - v_0) - (u_2 - u_0) * (v_1 - v_0)|;
 *      rho = ((ua2 * (float)W_0) * (float)H_0) / ((float)|area2| / 256.0f)  -- area2 is the frame's integer doubled area in 1/16
 *      pixel units, so rho is texels per sample;  l = 0; while (l < levels - 1 && rho > 2 * 4^l) ++l;  the nearest level: a NaN
 *      stays at 0 and +inf goes to the last level.  With use_mips = 0, l = 0.
 *   4. wrap (repeat): uw = u - floorf(u), vw = v - floorf(v);  x = uw * (float)W_l - 0.5f;  y = (1.0f - vw) * (float)H_l - 0.5f
 *      (row 0 is the image's top and v points up, the convention of m324_surface_sample's uv).
 *   5. bilinear: x0 = floorf(x), fx = x - x0; columns x0 mod W_l and (x0 + 1) mod W_l, taken non-negative; rows the same from y.
 *      Per channel on (float)byte, t_rc the tap at row r, column c of the pair:  top = t00 + fx * (t01 - t00);
 *      bot = t10 + fx * (t11 - t10);  val = top + fy * (bot - top);  albedo = val / 255.0f.  Bytes are used as they are (no
 *      sRGB decode), like colors and the samplers.
 *   Resolve: the byte of an output pixel is (sum over its ss x ss samples of the sample's byte + ss * ss / 2) >> log2(ss * ss) per
 *   channel; a background sample contributes the background byte.  One lane per output pixel walks its samples: no S' x S'
 *   colour buffer exists.  With face_uvs NULL and ss = 1 the three outputs equal m324_render_shade's bit for bit.
 * Every entry point validates its arguments before its first HIP call and then returns M324_ERR_INVALID with a message.
 * ------------------------------------------------------------------------------------------ */
#define M324_TEXTURE_MAX_SIDE 16384
#define M324_TEXTURE_MAX_LEVELS 15
int m324_texture_plan(int tex_h, int tex_w, int* levels, long* bytes);
int m324_texture_mips(const unsigned char* texels, int tex_h, int tex_w, int channels, void* mips, long mips_bytes, void* stream);
int m324_render_shade_tex(const int* faces, int n_faces, int n_vertices, int frames, int size, const float* colors, const float* normals,
                          long normal_stride_t, const float* view, float ambient, int background, const float* face_uvs,
                          const void* mips, int tex_h, int tex_w, int use_mips, int supersample, unsigned char* rgb, int* face,
                          int* depth, void* scratch, long scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Perceptual evaluation (csrc/perceptual.hip, and csrc/conv.hip for m324_conv3x3 and m324_maxpool2x2; added at ABI 23 without a
 * bump): the pieces of LPIPS on a VGG16 trunk, what motion324_amd/perceptual.py strings together.  replaces:
 * lpips.LPIPS(net='vgg', spatial=True) of the reference's evaluation/evaluation.py (torch / cuDNN there).  Everything is fp32,
 * activations are NHWC ([images, H, W, C], C contiguous), every pointer is device memory and 16-byte aligned unless said
 * otherwise, and images * H * W stays below 2^31.
 *
 * m324_conv3x3: m324_conv3x3_ex (below) restricted to one input tensor (a = in, Ca = Cin, b = NULL), dilation 1, no residual and
 *   Cout % 32 = 0 -- the same kernel behind the same host path, which words its refusals in Ca -- with a tile rule of its own
 *   that never shows in the bits:
 *   out[i, y, x, n] = act(bias[n] + sum over taps t = 3 (dy + 1) + (dx + 1), dy, dx in -1..1, and channels c of
 *   in[i, y + dy, x + dx, c] * wp[t * Cin + c][n]),  stride 1, a tap outside the image contributes 0 (zero padding of `in` itself),
 *   act = max(., 0) when relu = 1, the identity when relu = 0.
 *   Shape contract: Cin % 4 = 0, Cout % 32 = 0, both in 4 / 32 .. M324_CONV_MAX_CHANNELS; any H, W >= 1; any images >= 1.
 *   wp: the weights repacked K-major, [Kpad, Cout] with row k = t * Cin + c and Kpad = 9 Cin rounded up to a multiple of
 *   M324_CONV_KPAD; the rows from 9 Cin on are read and must hold zeros.  A 3-channel input is a 4-channel one whose fourth
 *   channel and fourth weight rows are zero (m324_lpips_prepare writes that input).
 *   Arithmetic: v_mfma_f32_32x32x2_f32, a sum in two levels.  r_j = the chain of fp32 fmas over k = j R .. min((j + 1) R, 9 Cin) - 1
 *   in that order starting from 0, one rounding per product, R = M324_CONV_RUN; s = ((0 + r_0) + r_1) + ... in order; the
 *   output is act(s + bias).  (One chain over all k loses accuracy with the length of the running sum: at 9 Cin = 4608 the
 *   metric's deep layers came out up to 10 times further from fp64 than with runs of 144.)  An output's bits depend on its
 *   9 Cin inputs and the weights alone: not on the image's place in the batch, the tile, the grid or a second call.
 * m324_maxpool2x2: out[i, y, x, c] = max of in[i, 2y .. 2y + 1, 2x .. 2x + 1, c]; H and W even, C % 4 = 0.  Exact.  The kernel of
 *   m324_maxpool2x2_ceil, which cuts no window at even sizes; odd sizes are refused here.
 * m324_lpips_prepare: the scaled input of the trunk, dst fp32 [images, H, W, 4]:  dst_c = (x_c - shift_c) / scale_c for c < 3 with
 *   shift (-.030, -.088, -.188), scale (.458, .448, .450), and dst_3 = 0.  mode M324_LPIPS_U8_NHWC: src uint8 [images, H, W, 3]
 *   (any alignment), x = ((float)v / 255) * 2 - 1.  mode M324_LPIPS_F32_NCHW: src fp32 [images, 3, H, W] (4-byte aligned),
 *   x = v, or v * 2 - 1 when normalize = 1.  Evaluated as written, nothing contracted: bytes and the floats built from them by
 *   the same formula give the same bits.
 * m324_lpips_layer: out[p] = (1 / pixels) sum over the pixels of sum_c w[c] (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2
 *   for pair p of fa, fb [pairs, pixels, channels], |f| = sqrt(sum_c f_c^2) over the pixel's channels; channels % 4 = 0,
 *   <= M324_LPIPS_MAX_CHANNELS; pixels <= 2^24.  partial: scratch of pairs * M324_LPIPS_CHUNKS floats.  No atomics: a pair's
 *   pixels are cut into min(M324_LPIPS_CHUNKS, ceil(pixels / 64)) equal runs, a workgroup sums one run in a fixed order, a second
 *   kernel adds a pair's runs in order and divides.  The order depends on (pixels, channels) only -- not on pairs or p -- and
 *   nothing is contracted, so swapping fa and fb gives the same bits and fa = fb gives exactly 0.
 * Every entry point validates its arguments before its first HIP call and then returns M324_ERR_INVALID with a message.
 * ------------------------------------------------------------------------------------------ */
#define M324_CONV_KPAD 16
#define M324_CONV_RUN 144
#define M324_CONV_MAX_CHANNELS 4096
#define M324_LPIPS_U8_NHWC 0
#define M324_LPIPS_F32_NCHW 1
#define M324_LPIPS_MAX_CHANNELS 1024
#define M324_LPIPS_CHUNKS 64
int m324_conv3x3(const float* in, const float* wp, const float* bias, float* out, int images, int H, int W, int Cin, int Cout, int relu,
                 void* stream);
int m324_maxpool2x2(const float* in, float* out, int images, int H, int W, int C, void* stream);
int m324_lpips_prepare(const void* src, int mode, int normalize, int images, int H, int W, float* dst, void* stream);
int m324_lpips_layer(const float* fa, const float* fb, const float* w, int pairs, long pixels, int channels, float* partial, float* out,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Foreground matting (csrc/matting.hip, and csrc/conv.hip for m324_conv3x3_ex, m324_conv3x3_ex_tile and m324_maxpool2x2_ceil;
 * added at ABI 23 without a bump): the pieces of U2-Net and of the arithmetic the `rembg` package wraps around it, what
 * motion324_amd/matting.py strings together.  replaces: the per-frame rembg.remove(frame, session='u2net') loop of the
 * reference's utils/inference_utils.py:segment_foreground_with_u2net (onnxruntime with a PIL round trip there).  Everything is fp32 unless said otherwise, activations are NHWC ([images, H, W, C],
 * C contiguous), every pointer is device memory and 16-byte aligned unless said otherwise, images * H * W stays below 2^31.
 *
 * m324_conv3x3_ex: the general 3 x 3 convolution, of which m324_conv3x3 is a restriction.  The input is the channel
 *   concatenation of a [images, H, W, Ca] and b [images, H, W, Cb] (a's channels first; b = NULL with Cb = 0 for one source),
 *   which is never built:
 *     s[i, y, x, n] = sum over taps t = 3 (dy + 1) + (dx + 1), dy, dx in -1..1, and channels c < Ca + Cb of
 *                     cat[i, y + dilation dy, x + dilation dx, c] * wp[t (Ca + Cb) + c][n],   a tap outside the image contributes 0,
 *     out = act(s + bias) + res  with act = max(., 0) when relu = 1 and res [images, H, W, Cout] optional (NULL: nothing added).
 *   Shape contract: Ca % 4 = Cb % 4 = 0, Ca >= 4, Ca + Cb <= M324_CONV_MAX_CHANNELS; Cout % 4 = 0 in 4..M324_CONV_MAX_CHANNELS;
 *   dilation in 1..M324_CONV_MAX_DILATION; any H, W, images >= 1.  wp [Kpad, Cout] as for m324_conv3x3 with Cin = Ca + Cb.  A
 *   convolution with fewer than four outputs (the side outputs: one) is packed with zero columns and a zero bias up to four.
 *   Arithmetic: that of m324_conv3x3, unchanged -- chains of M324_CONV_RUN consecutive k from 0 on v_mfma_f32_32x32x2_f32, the
 *   chains added in order, then + bias, the activation, + res (one rounding each).  With dilation 1, b = NULL and res = NULL the
 *   bits are those of m324_conv3x3 wherever that accepts the shape: it is the same kernel.  The tile (128 pixels by 128, 64 or
 *   32 channels) is chosen from Cout and the pixel count -- m324_conv3x3_ex_tile (host only) returns its width -- and never shows in the bits, nor does
 *   the image's place in the batch, the grid or a second call.
 * m324_maxpool2x2_ceil: out[i, y, x, c] = max of in[i, 2y .. min(2y + 1, H - 1), 2x .. min(2x + 1, W - 1), c], out [images,
 *   ceil(H / 2), ceil(W / 2), C]: MaxPool2d(2, 2, ceil_mode=True).  C % 4 = 0.  Exact.
 * m324_upsample_bilinear: in [images, H, W, C] -> out [images, Ho, Wo, C], bilinear with align_corners = false; C % 4 = 0, every
 *   size in 1..M324_MATTE_MAX_SIDE.  Per axis, in fp32 and in this order, nothing contracted:
 *     scale = (float)in / (float)out;  s = max(((float)o + 0.5f) * scale - 0.5f, 0);  i0 = min((int)s, in - 1);
 *     i1 = i0 + (i0 < in - 1);  l1 = min(max(s - (float)i0, 0), 1);  l0 = 1 - l1;
 *   and the value is  y.l0 * (x.l0 * v[y.i0][x.i0] + x.l1 * v[y.i0][x.i1]) + y.l1 * (x.l0 * v[y.i1][x.i0] + x.l1 * v[y.i1][x.i1]).
 *   Equal sizes copy the input exactly (l1 = 0).
 * m324_matte_prepare: src uint8 [images, H, W, 3] (dense, any alignment) -> dst fp32 [images, H, W, 4]:
 *   m = max(largest byte of the frame, 1e-6);  dst_c = (float)(((double)v_c / m - mean_c) / std_c) for c < 3, mean (.485, .456,
 *   .406), std (.229, .224, .225); dst_3 = 0.  Evaluated in float64 as written and rounded once: the bits numpy gets.
 *   frame_max: int [images], written (the per-frame maximum, an integer reduction); partial: scratch of images *
 *   M324_MATTE_CHUNKS ints.  The reduction has two levels -- a frame is cut into min(M324_MATTE_CHUNKS, ceil(n /
 *   M324_MATTE_CHUNK_ITEMS)) equal runs, a workgroup per run, a second kernel over a frame's runs -- so that a few frames fill the chip.
 * m324_matte_fuse: the fused side-output head.  sides, side_h, side_w: HOST arrays of M324_MATTE_SIDES device pointers and sizes,
 *   map k fp32 [images, side_h[k], side_w[k], side_stride] of which channel 0 is read (4-byte aligned); outconv: HOST array of
 *   M324_MATTE_SIDES weights and the bias.  Per output pixel of [images, Ho, Wo]: u_k = map k sampled as m324_upsample_bilinear
 *   samples it (side_h[k] <= Ho, side_w[k] <= Wo), d0 = ((((((0 + w_0 u_0) + w_1 u_1) + ...) + w_5 u_5) + bias, nothing contracted;
 *   prob = 1 / (1 + expf(-d0)); logit (optional) receives d0.
 * m324_matte_quantise: p fp32 [images, pixels] -> q uint8: per frame mi = min p, ma = max p (exact in any order; written to
 *   minmax fp32 [images, 2]), q = (uint8)(((p - mi) / (ma - mi)) * 255) in fp32 as written, truncated.  A frame with ma = mi
 *   (numpy: NaN) gives q = 0.  partial: scratch of images * M324_MATTE_CHUNKS * 2 floats, the two levels of m324_matte_prepare.
 *
 * ISNet (the IS-Net of DIS; `rembg`'s session 'isnet-general-use', which the reference's utils/rmbg_for_black_bg.py and
 * scripts/hunyuan_Gen.py select; added at ABI 23 without a bump) is built from the same blocks and needs three more pieces:
 * m324_conv3x3_s2: the stem, Conv2d(Cin, Cout, 3, stride=2, padding=1).  in [images, H, W, Cin] -> out [images, Ho, Wo, Cout] with
 *   Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1:
 *     out[i, y, x, n] = act(bias[n] + sum over taps t and channels c of in[i, 2y + dy, 2x + dx, c] * wp[t Cin + c][n]),
 *   a tap outside the image contributes 0.  Shape contract: m324_conv3x3_ex's for one source (Cin % 4 = 0, Cout % 4 = 0, any H, W,
 *   images >= 1; images * H * W below 2^31); wp as there.  It is the kernel of m324_conv3x3_ex with a compile-time gather: the same
 *   chains of M324_CONV_RUN consecutive k from 0 on v_mfma_f32_32x32x2_f32, added in order, then + bias, then the activation.  The
 *   tile is m324_conv3x3_ex's rule on the OUTPUT pixel count and never shows in the bits.  Consequence: with zero padding 1,
 *   conv3x3_s2(x) has the bits of conv3x3_ex(x)[:, ::2, ::2] (one source, dilation 1, no residual).
 * m324_matte_prepare_ex: m324_matte_prepare with given constants.  mean_std: HOST array of six doubles, mean_0..2 then std_0..2;
 *   dst_c = (float)(((double)v_c / m - mean_c) / std_c), in float64 as written; every std finite and above 0, every mean finite
 *   (checked on the host).  m324_matte_prepare is this call with (.485, .456, .406, .229, .224, .225): one kernel, the same bits.
 * m324_matte_side: the one-map head.  side fp32 [images, side_h, side_w, side_stride] of which channel 0 is read (4-byte aligned).
 *   Per output pixel of [images, Ho, Wo], Ho >= side_h, Wo >= side_w: d1 = that channel sampled by the rule of
 *   m324_upsample_bilinear, the same operations in the same order, nothing contracted -- the bits of channel 0 of its output,
 *   which is never written; prob = 1 / (1 + expf(-d1)); logit (optional) receives d1.
 * Every entry point validates its arguments before its first HIP call and then returns M324_ERR_INVALID with a message.  No
 * atomics anywhere: every result is a fixed sequence of operations.
 * ------------------------------------------------------------------------------------------ */
#define M324_CONV_MAX_DILATION 64
#define M324_MATTE_SIDES 6
#define M324_MATTE_MAX_SIDE 16384
#define M324_MATTE_CHUNKS 64
#define M324_MATTE_CHUNK_ITEMS 4096
int m324_conv3x3_ex(const float* a, int Ca, const float* b, int Cb, const float* wp, const float* bias, const float* res, float* out,
                    int images, int H, int W, int Cout, int dilation, int relu, void* stream);
int m324_conv3x3_ex_tile(int images, int H, int W, int Cout);
int m324_maxpool2x2_ceil(const float* in, float* out, int images, int H, int W, int C, void* stream);
int m324_upsample_bilinear(const float* in, float* out, int images, int H, int W, int Ho, int Wo, int C, void* stream);
int m324_matte_prepare(const unsigned char* src, int images, int H, int W, int* partial, int* frame_max, float* dst, void* stream);
int m324_matte_fuse(const float* const* sides, const int* side_h, const int* side_w, int side_stride, const float* outconv, int images,
                    int Ho, int Wo, float* prob, float* logit, void* stream);
int m324_matte_quantise(const float* p, int images, long pixels, float* partial, float* minmax, unsigned char* q, void* stream);
int m324_conv3x3_s2(const float* in, const float* wp, const float* bias, float* out, int images, int H, int W, int Cin, int Cout, int relu,
                    void* stream);
int m324_matte_prepare_ex(const unsigned char* src, int images, int H, int W, const double* mean_std, int* partial, int* frame_max, float* dst,
                          void* stream);
int m324_matte_side(const float* side, int side_h, int side_w, int side_stride, int images, int Ho, int Wo, float* prob, float* logit,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Video metric, FVD (csrc/conv3d.hip; added at ABI 23 without a bump): the pieces of an I3D trunk (Inception-v1 inflated to 3D)
 * from decoded frames to the 400 logits.  replaces: the detector call of the reference's evaluation/fvd/styleganv/fvd.py
 * (a TorchScript I3D on the framework's convolutions) and its preprocess_single.  All tensors fp32 NDHWC.
 *
 * Geometry shared by m324_conv3d and m324_maxpool3d: input [samples, T, H, W, .], a window (kt, kh, kw), per-axis strides (st, sh,
 *   sw) each 1 or 2, and an explicit FRONT padding (pt, ph, pw), 0 <= p < k.  The output is [samples, ceil(T / st), ceil(H / sh),
 *   ceil(W / sw), .]; output (t, h, w) reads the input voxels (t st - pt + dt, h sh - ph + dh, w sw - pw + dw), 0 <= d < k.  The
 *   TensorFlow "SAME" rule is the caller's: total = max(k - s, 0) if n % s == 0 else max(k - n % s, 0), front = total / 2.
 *   samples * T * H * W stays below 2^31.
 * m324_conv3d: out[v, n] = act(bias[n] + sum over taps and channels c of a[voxel(v, tap), c] * wp[tap Cin + c][n]); a voxel outside
 *   the volume contributes 0.  The tap box is (1,1,1), (3,3,3) or (7,7,7), given by its side `box`; tap = (dt box + dh) box + dw.
 *   a is a channel slice: channel c of voxel v at a[v lda + c], Cin % 4 = 0, lda % 4 = 0, lda >= Cin; out likewise with ldo and
 *   Cout, Cout % 8 = 0: channels outside [0, Cout) of the ldo-wide rows are not written.  wp [Kpad, Cout] dense, Kpad = box^3 Cin
 *   rounded up to M324_CONV_KPAD, the rows behind box^3 Cin read and zero.  A 3-channel input is a 4-channel one with zero
 *   weights for the fourth (m324_fvd_prepare writes that input).
 *   Arithmetic: m324_conv3x3's -- chains of M324_CONV_RUN consecutive k from 0.0f on v_mfma_f32_32x32x2_f32, one rounding per
 *   product, the chains added in order from 0, then + bias, then max(., 0) when relu.  The same sequence for an output whatever
 *   its place in tile, grid or batch and whatever the tile: `tile` 0 lets the library choose (m324_conv3d_tile, host only, returns
 *   that choice for an output voxel count), 32, 64 or 128 force a width, and the bits are the same.  Consequence: the output of
 *   stride 2 along an axis equals every second voxel along it of the stride-1 output with the same front padding.
 * m324_maxpool3d: windows (1,3,3), (3,3,3) and (2,2,2); the maximum runs over the window's voxels INSIDE the volume: padding is
 *   excluded (the original model's semantics; it equals the zero-padded pool of the PyTorch ports wherever the pooled map is
 *   non-negative, as every map the network pools is, behind a ReLU).  in dense [.., C], C % 4 = 0; out a channel slice (ldo).  Exact.
 * m324_i3d_head: x [samples, T, hw, hw, C] dense, T >= 2 -> out [samples, classes]:
 *     pooled[n, t, c] = (((0 + x[n, t, 0, 0, c]) + x[n, t, 0, 1, c]) + ... over (dt in {0, 1}, h, w), dt slowest) / (2 hw hw),
 *       t in 0..T - 2 (pooled: scratch of samples * (T - 1) * C floats);
 *     logit[n, t, j] = ((q0 + q1) + (q2 + q3)), q_r the fma chain from 0.0f over the channels c = r mod 4 in order of
 *       pooled[n, t, c] * w[c, j], w [C, classes];
 *     out[n, j] = (sum over t in order from 0 of (logit[n, t, j] + b[j])) / (T - 1).
 *   Nothing else is contracted; no atomics: a sample's result does not depend on the batch.
 * m324_fvd_prepare: src [frames, H, W, 3], uint8 (M324_FVD_U8, u = (float)v / 255.0f) or fp32 in [0, 1] (M324_FVD_F32, u = v), dense
 *   -> dst fp32 [frames, Ho, Wo, 4].  Pixel (y, x) of dst is pixel (y + y0, x + x0) of the bilinear resize of the frame to Hr x Wr
 *   (align_corners = false, no antialiasing; per axis and in combination the rule and order of m324_upsample_bilinear, on u),
 *   then (r - 0.5f) * 2.0f, nothing contracted; channel 3 is 0.  Hr = H and Wr = W copy u exactly.  The reference's
 *   preprocess_single is the call with the shorter side scaled to 224, the longer to ceil, and the centre 224 x 224 crop
 *   (ops.fvd_geometry computes it).
 * Every entry point validates its arguments before its first HIP call and then returns M324_ERR_INVALID with a message.
 * ------------------------------------------------------------------------------------------ */
#define M324_CONV3D_MAX_STRIDE 16384
#define M324_I3D_HEAD_MAX_SAMPLES 65536
#define M324_I3D_HEAD_MAX_SIDE 64
#define M324_FVD_U8 0
#define M324_FVD_F32 1
int m324_conv3d(const float* a, long lda, const float* wp, const float* bias, float* out, long ldo, int samples, int T, int H, int W, int Cin,
                int Cout, int box, int st, int sh, int sw, int pt, int ph, int pw, int relu, int tile, void* stream);
int m324_conv3d_tile(long voxels, int Cout);
int m324_maxpool3d(const float* in, float* out, long ldo, int samples, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw,
                   int pt, int ph, int pw, void* stream);
int m324_i3d_head(const float* x, const float* w, const float* b, float* pooled, float* out, int samples, int T, int hw, int C, int classes,
                  void* stream);
int m324_fvd_prepare(const void* src, int mode, long frames, int H, int W, int Hr, int Wr, int y0, int x0, int Ho, int Wo, float* dst,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * A plain ViT image tower in fp32 (csrc/vit.hip; added at ABI 23 without a bump): what open_clip's VisionTransformer needs
 * besides m324_gemm -- heads of any width, rows wider than 1024, byte images under another normalisation.
 *   replaces: model.encode_image of open_clip's ViT-bigG-14 at evaluation/calculate_lpips.py:90-136 (the "CLIP Loss" line of
 *             evaluation/evaluation.py), together with m324_gemm and m324_frame_resample; motion324_amd/clipsim.py is the host.
 * m324_attention_tok: O = softmax(q k^T * scale) v per (batch, head), fp32, straight from the token-major result of a fused
 *   in-projection (nn.MultiheadAttention.in_proj order): row b * L + l of qkv (ld elements apart) holds q in columns
 *   [h * D, (h + 1) * D), k in H * D + the same and v in 2 * H * D + the same.  O[(b * L + l) * ldo + h * D + d]; nothing else of
 *   O is written.  No split pass, no transposed V and no padding in HBM.  D % 8 == 0, 8 <= D <= 128 (else
 *   M324_ERR_UNSUPPORTED); ld >= 3 * H * D and ldo >= H * D, both multiples of 4; bases 16-byte aligned; L >= 1; scale > 0.
 *   The arithmetic is m324_attention's fp32 kernel: scores as k-ordered fp32 fma chains (v_mfma_f32_32x32x2_f32), a running
 *   maximum over key tiles, exp2f of (score * scale * log2(e) - maximum), fp32 sums, one division per row.
 * m324_layernorm_wide: m324_layernorm's arithmetic (the mean, then the sum of squared deviations from it) on fp32 in and out
 *   for C % 4 == 0, 4 <= C <= 4096 (else M324_ERR_UNSUPPORTED); ldx, ldy multiples of 4 and >= C; b may be NULL; y must not
 *   overlap x.  No row map: a strided selection of rows is a larger ldx (the class-token rows of a [n, L, C] stream: ldx = L * C).
 * m324_vit_patches: img [F, S, S, 3] uint8 -> out fp32 [F * g * g, Kp], g = S / patch; column c * patch * patch + ky * patch + kx
 *   (the Conv2d weight's flattening) holds ((float)v / 255.0f - mean[c]) / std[c], each operation one IEEE fp32 operation in
 *   that order (torchvision's ToTensor, then Normalize); columns 3 * patch * patch .. Kp - 1 are zero.  Kp % 32 == 0 (else
 *   M324_ERR_UNSUPPORTED).  mean_std: six floats in DEVICE memory, the three means, then the three standard deviations.
 * m324_vit_tokens: x [F * L, C] from patch_rows [F * (L - 1), C], cls [C] and pos [L, C]: x[f * L] = cls + pos[0],
 *   x[f * L + 1 + p] = patch_rows[f * (L - 1) + p] + pos[1 + p], one fp32 addition per element.  C % 4 == 0; all dense.
 * ------------------------------------------------------------------------------------------ */
int m324_attention_tok(const float* qkv, long ld, float* O, long ldo, int B, int L, int H, int D, float scale, void* stream);
int m324_layernorm_wide(const float* x, long ldx, const float* w, const float* b, float eps, float* y, long ldy, int rows, int C,
                        void* stream);
int m324_vit_patches(const unsigned char* img, int F, int S, int patch, const float* mean_std, float* out, int Kp, void* stream);
int m324_vit_tokens(const float* patch_rows, const float* cls, const float* pos, float* x, int F, int L, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Float resize and fp32 patch rows (csrc/vit.hip; added at ABI 23 without a bump): what DreamSim's three ViT-B/16 towers need in
 * front of them.  replaces: transforms.Resize((224, 224)) on a float tensor at evaluation/calculate_lpips.py:34-87 -- F.interpolate(
 * mode="bilinear", align_corners=False, antialias=True) on fp32 values, no 8-bit step -- and the towers' Normalize;
 * motion324_amd/dreamsim.py is the host and builds the tables (resize_tables, float64 rounded once to fp32).
 * m324_resample_f32: ONE separable pass.  src is uint8 [F, H, W, 3] (src_u8 != 0; a sample is (float)v / 255.0f, one IEEE fp32
 *   division: ToTensor) or fp32 planar [F, 3, H, W]; dst is fp32 planar, [F, 3, H, n_out] for axis 0 (x) and [F, 3, n_out, W] for
 *   axis 1 (y).  weights fp32 [n_out, ksize] and first int32 [n_out] in DEVICE memory: output o is the fp32 fma chain
 *   acc = fmaf(weights[o][k], sample(first[o] + k), acc), k = 0 .. ksize - 1 in that order from acc = 0; taps at or past the end
 *   of the axis are skipped (their weights are the zeros behind a row's taps).  Deterministic: no atomics, no order left to the
 *   hardware; the vectorised forms (16-byte stores; for the y pass 16-byte fp32 loads and 12-byte groups of four byte pixels,
 *   when W % 4 == 0 and the bases are 16-byte aligned) run the same chains.  first[o] must lie in [0, n_in): the kernel clamps
 *   it, so a bad table cannot read outside the source.  1 <= ksize <= 64; sides 1 .. 16384; dst must not overlap src.
 * m324_vit_patches_f32: m324_vit_patches from img fp32 planar [F, 3, S, S]: column c * patch * patch + ky * patch + kx of row
 *   f * g * g + py * g + px holds (img[f][c][py * patch + ky][px * patch + kx] - mean[c]) / std[c], two IEEE fp32 operations in
 *   that order (Normalize); columns 3 * patch * patch .. Kp - 1 are zero.  Kp % 32 == 0 (else M324_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------------ */
int m324_resample_f32(const void* src, int src_u8, int F, int H, int W, int axis, const float* weights, const int* first, int ksize,
                      int n_out, float* dst, void* stream);
int m324_vit_patches_f32(const float* img, int F, int S, int patch, const float* mean_std, float* out, int Kp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Volumetric IoU (csrc/voxel.hip; added at ABI 23 without a bump): exact surface voxelisation of `frames` poses of one
 * topology into a bit grid, the orthographic fill of such a grid, and the popcounts of two grids.  replaces: compute_iou_voxel
 * of the reference's evaluation/evaluation_pcd.py:612-637 (trimesh's subdivision voxeliser on the CPU; the reference keeps the call
 * commented out).  The arithmetic below IS the contract: which voxels a triangle marks is decided in integers and marking is a
 * 32-bit atomic OR, which is idempotent and commutes, so no output depends on arrival order, grid, CU count, queue order or
 * big_voxels.  Every result is an integer; the quotient of the IoU is formed by the caller.
 *
 * Grid: R = resolution, voxels per unit length (pitch 1 / R); H = half, the integer half extent: the grid covers [-H, H)^3 with
 *   G = 2 H R voxels per axis ("side").  R is a multiple of 16, so G is a multiple of 32; M324_VOXEL_MIN_SIDE <= G <=
 *   M324_VOXEL_MAX_SIDE.  Voxel (i, j, k) along x, y, z is the CLOSED cube [16 i, 16 i + 16] x [16 j, 16 j + 16] x [16 k, 16 k + 16]
 *   in sub-voxel units (1/16 voxel).  Occupancy is int32 words [frames, G, G, G / 32]: voxel (i, j, k) of frame t is bit i % 32 of
 *   word ((t G + k) G + j) (G / 32) + i / 32, read as unsigned.
 * Sizes: frames >= 1; n_vertices >= 1; n_faces >= 0; frames * n_faces < 2^31 and frames * n_vertices < 2^31.  vertices fp32, frame t
 *   at vertices + t * stride_t (ELEMENTS), vertex v at + 3 v.  faces int32 [n_faces, 3], shared by every frame; a face with an
 *   index outside [0, n_vertices) marks nothing (the Python wrappers refuse such faces before any launch).
 *
 * Snap, per frame and vertex, for each coordinate c of (x, y, z):
 *   q_c = rint(clamp((x_c + (float)H) * (float)(16 R), -131072, 131072))
 *   in uncontracted fp32, with clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v) and rint = round to nearest, ties to even (as in
 *   m324_render_project).  A vertex with a non-finite coordinate is invalid and every triangle that touches it is skipped.
 *   outside[t] counts the valid vertices of frame t with some q_c outside [0, 16 G]: geometry the grid does not hold.
 *
 * Overlap.  A triangle with integer vertices v_0, v_1, v_2 marks voxel (i, j, k) iff none of 13 axes separates it from the
 *   voxel's closed cube, all in int64.  c = (16 i + 8, 16 j + 8, 16 k + 8), v'_m = v_m - c; e_0 = v_1 - v_0, e_1 = v_2 - v_1,
 *   e_2 = v_0 - v_2.
 *   - the three cube axes a: separated iff min_m v'_ma > 8 or max_m v'_ma < -8;
 *   - the normal n = e_0 x e_1: separated iff |n . v'_0| > 8 (|n_x| + |n_y| + |n_z|);
 *   - for each edge e_m and each unit axis u: a = e_m x u, p_l = a . v'_l, r = 8 (|a_x| + |a_y| + |a_z|); separated iff
 *     min_l p_l > r or max_l p_l < -r.
 *   Touching counts: a triangle that lies in the plane between two voxel layers marks both.  Degenerate triangles (a segment, a
 *   point) go through the same 13 tests, which stay exact for them: no special case.  A voxel outside [0, G)^3 is not marked.
 *   Bounds: |q_c| <= 2^17, edge components <= 2^18, |c_a| < 2^15, so |v'| < 2^18; components of n <= 2^37, 8 (|n_x| + |n_y| + |n_z|)
 *   < 2^42, and every projection (n . v'_0, a . v'_l) stays below 2^57: this is where G <= 1024 and the clamp come from.
 * Work distribution (never visible in the result): the voxels that pass the three cube axes, clipped to [0, G - 1] per axis,
 *   form the triangle's box.  An empty box marks nothing.  A box of at most big_voxels (>= 0) voxels is walked by the lane that
 *   loaded the triangle; the others are appended to a queue of capacity frames * n_faces (one counter add per wave) and a second
 *   launch gives each entry a whole workgroup, lanes striding over the box's words.  The bits a walk finds for one word leave in one
 *   no-return 32-bit atomic OR.  No workgroup waits for another; every loop is bounded by a clipped box or by the queue's capacity.
 *
 * m324_voxel_plan: host-only; validates the sizes and stores the scratch bytes of m324_voxelize in *scratch_bytes (may be NULL).
 * m324_voxelize: ZEROES grid (int32 [frames, G, G, G / 32]) and outside (int32 [frames]) on the stream, then snaps and marks; the
 *   caller zeroes nothing.  scratch: device memory, 16-byte aligned, m324_voxel_plan bytes for the same sizes.
 * m324_voxel_fill: the rule usually called orthographic fill.  E_x(i, j, k) is true iff occupied voxels exist at some i1 <= i and
 *   some i2 >= i in row (j, k) of the frame; E_y and E_z the same along their axes; out = E_x & E_y & E_z, which contains the
 *   surface.  It is NOT a flood fill: a cup without a lid stays empty (nothing above its inside), but under a lid that covers
 *   half of it the inside is filled, although it is connected to the outside.  Along x this is bit
 *   arithmetic within a row of words, along y and z a forward and a backward OR scan per column of words.  out is a second grid
 *   that does not overlap `grid` (scratch may be NULL), or `grid` itself: then scratch is device memory of the grid's size
 *   (4 frames G^3 / 32 bytes, 4-byte aligned) and the result is copied back on the stream.
 * m324_voxel_counts: counts int64 [frames, 3] = (|A|, |B|, |A & B|) of two grids by popcount; a and b 16-byte aligned; frames <=
 *   65535.  counts is zeroed on the stream; each workgroup reduces its share and issues one 64-bit integer atomic add per
 *   number: integer addition commutes, so the counts are deterministic.  The caller forms union = |A| + |B| - |A & B| and
 *   iou = |A & B| / union in fp64, 0.0 when union = 0 (as the reference does).
 * Every entry point validates its arguments before its first HIP call and then returns M324_ERR_INVALID with a message.
 * ------------------------------------------------------------------------------------------ */
#define M324_VOXEL_MIN_SIDE 32
#define M324_VOXEL_MAX_SIDE 1024
int m324_voxel_plan(int n_vertices, int n_faces, int frames, int resolution, int half, long* scratch_bytes);
int m324_voxelize(const float* vertices, long stride_t, int n_vertices, const int* faces, int n_faces, int frames, int resolution, int half,
                  int big_voxels, int* grid, int* outside, void* scratch, long scratch_bytes, void* stream);
int m324_voxel_fill(const int* grid, int* out, int frames, int side, void* scratch, long scratch_bytes, void* stream);
int m324_voxel_counts(const int* a, const int* b, int frames, int side, long* counts, void* stream);

/* ==========================================================================================
 * Training-side entry points (backward of the path; reference: torch autograd over the same modules,
 * train.py:150-166).  The backward GEMMs reuse m324_gemm on transposed operands:
 *   dA[M,K] = dC[M,N] . Wt[K,N]^T          (Wt = m324_transpose(W))
 *   dW[N,K] (+)= dCt[N,Mp] . At[K,Mp]^T    (dCt, At = m324_transpose of the activations, Mp = round_up(M,64))
 * ========================================================================================== */
/* out[c][r] = in[r][c] for r < rows, zeros for rows <= r < rows_pad.  out is [cols, ld_out >= rows_pad]. */
int m324_transpose(const void* in, long ld_in, void* out, long ld_out, int rows, int cols, int rows_pad,
                   int dtype, void* stream);
/* out[c] (+)= sum over rows of x[r][c] (fp32 accumulation): bias gradients. */
int m324_colsum(const void* x, long ld, float* out, int rows, int cols, int dtype, int accumulate,
                float* scratch, int scratch_rows, void* stream);
/*   scratch (optional, scratch_rows x cols floats): lets tall inputs be reduced by row chunks in parallel. */
/* Many fp32 column sums in ONE launch (ABI 20): the split-K partials of the weight gradients, the per-workgroup partials of
 * the LayerNorm / RMSNorm weight gradients -- ~350 m324_colsum launches of a training step (train.py:166) become ~40.
 *   items[i]: dst[c] (+)= sum over rows of src[r * ld + c], c < cols.  chain = 1: the item CONTINUES item i - 1 (same dst, same
 *   cols): its sum is added to the running value by the same thread right behind it -- exactly what consecutive m324_colsum
 *   calls with accumulate = 1 compute, in the same order (deterministic; bit-identical to them for rows <= 64).
 *   Up to 64 items per launch (the table travels in the kernel arguments; longer lists are cut into several launches). */
typedef struct {
    float* dst;
    const float* src;
    long ld;
    int rows, cols;
    int accumulate;
    int chain;
} m324_colsum_item;
int m324_colsum_multi(const m324_colsum_item* items, int n, void* stream);
/* h = gelu_erf(z);  dz = dh * gelu'(z)  (nn.GELU, transformer.py:58), elementwise over n values. */
int m324_gelu(const void* z, void* h, long n, int dtype, void* stream);
int m324_gelu_bwd(const void* z, const void* dh, void* dz, long n, int dtype, void* stream);
/* LayerNorm backward (weight-only or with bias; the statistics are recomputed from x):
 *   dx[in_row(r)] (+)= d/dx ; the launch has n_partial workgroups of 8 waves (one row per wave at a time) and
 *   partial[n_partial][2C] receives every workgroup's sums of dy*xhat | dy -- reduce with
 *   m324_colsum(partial, 2C, ..., rows = n_partial) to get dw | db (fixed order = deterministic). */
int m324_layernorm_bwd(const float* x, long ldx, const float* w, float eps, const void* dy, long ldy, int dy_dtype,
                       float* dx, long lddx, int accumulate, float* partial, int n_partial, int rows, int C,
                       int gin, int gout, int off, void* stream);
/* The same, and in the same pass: dx_bf16[in_row(r)] = the resulting dx row rounded to bf16 (what the backward GEMMs behind it
 * read -- the reference's autograd hands the fp32 gradient to a bf16 autocast Linear the same way), and partial gets a THIRD
 * block: partial[n_partial][3C] = dy*xhat | dy | column sums of the rounded dx (the bias gradient of the Linear whose output
 * gradient this dx is).  Replaces m324_cast + m324_colsum over the tensor after every LayerNorm backward of the training step. */
int m324_layernorm_bwd_cast(const float* x, long ldx, const float* w, float eps, const void* dy, long ldy, int dy_dtype,
                            float* dx, long lddx, int accumulate, float* partial, int n_partial, int rows, int C,
                            int gin, int gout, int off, void* dx_bf16, long ldc, void* stream);

/* out = in converted between fp32 / bf16 (rows x cols, leading dims in elements). */
int m324_cast(const void* in, long ld_in, int in_dtype, void* out, long ld_out, int out_dtype, int rows, int cols,
              void* stream);
/* Attention backward (flash-attention backward of transformer.py:134-139,209-214 under autograd).
 *   m324_attention_delta: D[B,H,L] = rowsum(dO * O) over each head's 64 columns (token-major O, dO, ld >= H*64).
 *   m324_attention_bwd:   Qs[Bq,H,Lq,64] (pre-scaled q, q_bstride 0 = shared), K, V [B,H,Lk,64] row-major, dO [B,H,Lq,64]
 *                         head-major, lse / D [B,H,Lq] -> dQ [B,H,Lq,64] (w.r.t. the UNSCALED normalised q; per batch even when
 *                         q is shared: sum over batches afterwards), dK, dV [B,H,Lk,64].  fp32 arithmetic. */
int m324_attention_delta(const void* O, const void* dO, long ld, float* D, int B, int H, int L, int dtype, void* stream);
int m324_attention_bwd(const void* Qs, long q_bstride, const void* K, const void* V, const void* dO, const float* lse,
                       const float* D, void* dQ, void* dK, void* dV, int B, int H, int Lq, int Lk, float scale,
                       int dtype, void* stream);
/* bf16 MFMA implementation of the same backward (two kernels: dQ per query block, dK/dV per key block, both
 * recomputing the scores).  Besides the row-major operands it takes the transposed, permuted copies m324_qkv_split
 * emits: Qst [Bq,H,64,Lqp], Kt [B,H,64,Lkp], dOt [B,H,64,Lqp] (qt_bstride / q_bstride = 0 for a shared query set). */
int m324_attention_bwd_mfma(const void* Qs, const void* Qst, long q_bstride, long qt_bstride, const void* K, const void* Kt,
                            const void* V, const void* dO, const void* dOt, const float* lse, const float* D,
                            void* dQ, void* dK, void* dV, int B, int H, int Lq, int Lk, float scale, void* stream);
/* Backward of m324_qkv_split: head-major dQ/dK/dV -> token-major gradients of the projections (RMSNorm backward for
 * q, k when q_w / k_w are given; raw projections needed).  partial [n_partial][128]: per-block sums of the q_norm | k_norm
 * weight gradients, reduce with m324_colsum. */
int m324_qkv_split_bwd(const void* dQ, const void* dK, const void* dV, const void* q_raw, long ldq, const void* k_raw,
                       long ldk, const float* q_w, const float* k_w, float eps, void* dq_out, long ldoq, void* dk_out,
                       long ldok, void* dv_out, long ldov, float* partial, int n_partial, int B, int L, int H, int dtype,
                       void* stream);
/* Backward of m324_linear_n3: dA[M,K] = dout[M,3] . W[3,K]; partial [n_partial][3*K] = per-block sums of dout^T A
 * (reduce with m324_colsum to get dW).  mul (optional, ABI 22; A's dtype, [M, ldmul]): dA[m,k] is multiplied by mul[m,k] --
 * with the gelu'(z) the head's first Linear left (M324_AUX_STORE_GELU_GRAD) the kernel delivers d(pre-activation) directly and
 * the m324_gelu_bwd pass over the tensor is gone. */
int m324_linear_n3_bwd(const void* A, long lda, const float* W, const float* dout, void* dA, long ldda, float* partial,
                       int n_partial, int M, int K, int dtype, const void* mul, long ldmul, void* stream);
/* d[i] = coef * (*grad_scale) * (pred[i] - target[i])  -- backward of m324_mse (coef = 2 * weight / n). */
int m324_mse_bwd(const float* pred, const float* target, const float* grad_scale, float coef, float* d, long n,
                 void* stream);
/* torch.optim.AdamW step on one tensor (utils/training_utils.py:38-52: betas (0.9, 0.95), eps 1e-8, decoupled decay);
 * grad_scale: optional device scalar multiplying the gradient (clipping coefficient, train.py:196). */
int m324_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
               float weight_decay, int step, const float* grad_scale, void* stream);
/* The same update over the optimizer's WHOLE flat parameter buffer in one launch (multi-tensor semantics of
 * torch.optim.AdamW(fused=True), utils/training_utils.py:52): elements [0, n_decay) take `weight_decay` (parameters with
 * dim() > 1, training_utils.py:39-47), elements [n_decay, n) take none.  n, n_decay multiples of 4; 16-byte aligned. */
int m324_adamw_flat(float* p, const float* g, float* m, float* v, long n, long n_decay, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, const float* grad_scale, void* stream);
/* bf16 copies of the optimizer's flat fp32 parameter buffer in ONE launch (ABI 21): for every item (a Linear weight [rows, cols], cols a
 * multiple of 64, src_off -- a multiple of 4 -- elements into `src`) the row-major copy at dst + dst_off (the forward GEMM's operand) and, when dstT_off >= 0, the
 * transposed copy [cols, ldT] at dstT + dstT_off (the dgrad GEMM's operand; columns [rows, ldT) receive nothing but zeros: the caller
 * zeroes the buffer once).  Round to nearest even, as torch's .to(bfloat16).  items_dev: DEVICE memory (the table is constant
 * between optimizer steps), ordered by first_tile = the number of 64 x 64 tiles in front of the item; n_tiles = their total.
 *   replaces: the per-step torch casts + m324_transpose launches of every weight after optimizer.step()
 *             (train.py:203-213: the reference's autocast re-casts each weight inside every Linear call instead). */
typedef struct m324_mirror_item {
    long src_off, dst_off, dstT_off;
    long first_tile;
    int rows, cols, ldT, pad_;
} m324_mirror_item;
int m324_weight_mirror(const float* src, void* dst, void* dstT, const m324_mirror_item* items_dev, int n_items, long n_tiles,
                       void* stream);
/* *out (+)= sum g^2 (gradient-norm pieces); sanitize != 0 first applies nan_to_num(0, 1e-6, -1e-6) in place
 * (train.py:181-183).  partial: >= 1024 floats of scratch. */
int m324_grad_sumsq(float* g, long n, int sanitize, float* partial, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Collectives of the path over RCCL / xGMI (one process per GPU).
 *   replaces: the NCCL collectives torch.distributed issues for the reference -- DDP's gradient all-reduce
 *             (train.py:88-89,159-166; setup.py:134-140 creates the process group) -- and carries the two exchanges of the
 *             multi-GPU inference modes (k|v all-gather per global block, final [T, N, 3] all-gather).
 *   The Python host of this repo keeps using torch.distributed ("nccl" IS RCCL on ROCm) because the reference's callers
 *   own that process group; these entry points give a torch-free host the same collectives.  RCCL is resolved when
 *   m324_comm_init is first called (symbols already in the process, else librccl.so): libm324.so itself does not link it.
 *   Bootstrap: rank 0 calls m324_comm_unique_id and hands the 256-character hex string to the other ranks (file, env,
 *   socket -- the caller's business); every rank then calls m324_comm_init on ITS device (hipSetDevice first).
 *   All calls only enqueue on `stream`; buffers are device pointers; dtype M324_F32 / M324_BF16.
 * ------------------------------------------------------------------------------------------ */
typedef struct m324_comm m324_comm;
int m324_comm_unique_id(char* hex, int n);                         /* n >= 257 */
int m324_comm_init(m324_comm** comm, const char* unique_id_hex, int rank, int world);
/* in place; average != 0 divides by the number of ranks (DDP's gradient mean) */
int m324_comm_allreduce(m324_comm* comm, void* buf, long count, int dtype, int average, void* stream);
/* recv[r * count_per_rank ...] = rank r's send (rank order = frame order in the frame-parallel forward) */
int m324_comm_allgather(m324_comm* comm, const void* send, void* recv, long count_per_rank, int dtype, void* stream);
int m324_comm_destroy(m324_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* M324_H */
