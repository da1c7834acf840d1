/* espnet_mi355.h — C ABI of libespnet_mi355.so, the MI355X (gfx950) kernels behind
 * espnet_slurp_amd's drop-in ESPnet2 ASR training step.
 *
 * Conventions (every entry point):
 *   - plain device pointers (fp32 unless stated; int64 token ids as `long long`), sizes as int/long;
 *   - row-major, the layouts documented per function;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously, nothing syncs;
 *   - return 0 on success, non-zero on a launch/argument error; esp_last_error() describes it
 *     (thread-local).  No allocation happens inside: callers pass workspaces.
 *
 * Which reference interface each entry point replaces (BriansIDP/espnet_slurp, file:line):
 *   the reference has no native code on this path; these functions replace
 *   the ATen ops its Python building blocks call.  The reference-side "binding" is the espnet2
 *   plugin registry (espnet2/tasks/asr.py:133-188); see INTEGRATION.md.
 */
#ifndef ESPNET_MI355_H
#define ESPNET_MI355_H
#ifdef __cplusplus
extern "C" {
#endif

const char* esp_last_error(void);
int esp_abi_version(void);

/* ---- MFMA GEMM (nn.Linear fwd/bwd, Conv1d k=1, Conv2d via implicit im2col, attention
 * matmuls; attention.py:55-58,112,200-205, positionwise_feed_forward.py:32,
 * convolution.py:70-77, subsampling.py:84-85).
 *   C[z](m,n) = alpha*epi(sum_k A(m,k) B(k,n) + bias[n]) + beta*R[z](m,n)
 *   mode 0 (KC): elem(r,k)=p[r*ld+k]   mode 1 (RC): elem(r,k)=p[k*ld+r]
 *   mode 2/3: im2col of an NHWC map (3x3, stride 2); im2col_x = {H, W, C, Ho, Wo}
 *   z = z1*nb2+z2 ; operand offset = z1*s1 + z2*s2
 *   act: 0 none, 1 ReLU, 2 Swish (pre-activation stored to aux if non-NULL); dropout with
 *   probability drop_p keyed by (seed, (z*M+m)*N+n).  Every dropout site of this ABI rounds
 *   drop_p to the nearest multiple of 1/65536 (at least 1/65536 when drop_p > 0: a positive p
 *   never turns dropout off) and scales kept values by 1 / (1 - rounded p), so E[out] = in.
 *   bwd_act != 0 (backward of h = drop(act(pre)), positionwise_feed_forward.py:32): the
 *   epilogue is  v = drop'(acc + bias) * act'(pre)  with the dropout mask regenerated from
 *   (drop_p, seed); act must be 0 and aux NULL.
 *   rowsum != NULL (mode_a RC, batch 1): rowsum[m] += sum_k A(m,k) — the bias gradient of a
 *   weight-gradient GEMM (dW = dy^T x, db = colsum dy) in the same pass over dy.
 *   work/work_bytes: optional scratch; when the tile grid is too small to fill the chip the
 *   K range is split over blocks and reduced (fixed order, deterministic) before the epilogue.
 *   The last 64 KiB of work (work_bytes > 64 KiB) hold the split-K arrival tickets of the
 *   in-kernel combine: the caller zero-fills them once before the first call that uses this
 *   workspace and every launch leaves them zero; one workspace must not serve two launches
 *   that run concurrently (e.g. on two streams). */
int esp_gemm_f32(int mode_a, int mode_b, int M, int N, int K, int batch, int nb2,
                 const float* A, long lda, long sa1, long sa2,
                 const float* B, long ldb, long sb1, long sb2,
                 float* C, long ldc, long sc1, long sc2,
                 const float* bias, float alpha, float beta, const float* R,
                 int act, float* aux, float drop_p, unsigned long long seed,
                 int bwd_act, const float* pre, float* rowsum,
                 const int* im2col_a, const int* im2col_b, float* work, long work_bytes,
                 void* stream);
/* GEMM compute type for every later esp_gemm_f32 launch (process-wide host state, read at
 * launch time, so a captured HIP graph keeps the kernels of its capture): 0 = fp32 MFMA
 * (default; the reference's train_dtype float32), 1 = bf16 operands (fp32 values rounded to
 * nearest-even while staged into LDS) with fp32 accumulate and fp32 epilogue / outputs.
 * Mode 1 is the reduced-precision training path of SURVEY §8(d) C5; the reference's nearest
 * knob is `use_amp` (fp16 autocast, trainer.py:181-195,554).  Returns the previous value. */
int esp_set_gemm_compute(int dtype);
int esp_get_gemm_compute(void);
/* How the fp32 compute type (0) multiplies in the LDS-DMA GEMM kernel of this build: 6 = each
 * fp32 operand split exactly into three bf16 (hi + mid + lo, round-to-nearest-even residuals)
 * and the six products down to 2^-16 relative (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid)
 * accumulated in fp32 on v_mfma_f32_32x32x16_bf16 (the dropped terms are <= 2^-23 |a b|, below
 * an fp32 rounding of the sum); 1 = v_mfma_f32_32x32x2_f32 (build flag ESP_F32_SPLIT=0). */
int esp_f32_gemm_products(void);
/* Split-K combine of every later esp_gemm_f32 launch (process-wide): 0 = a separate
 * fixed-order reduction launch (default), 1 = in-kernel (the last-arriving unit of each output
 * tile sums the splits in fixed order; needs the zeroed ticket area of `work`, see above).
 * Initialised from ESP_SPLITK_INKERNEL.  Returns the previous mode. */
int esp_set_splitk_mode(int mode);
/* ABI 39.  The kernel of the fp32 RC x RC GEMMs with a plain epilogue (the Linear weight gradients, dW += dy^T x
 * with the fused bias gradient) of every later esp_gemm_f32 launch (process-wide): 1 (default) = the
 * warp-specialised kernel (csrc/gemm_wgrad_ws.hip: 256 x 128 tiles, operands split once per block on producer
 * waves) when M >= 256 and K is long enough for its split-K grid to fill the chip; 2 = that kernel for every
 * structurally eligible launch (unbatched, M % 4 == N % 4 == 0, LDS-DMA-eligible operands, split K or row sums);
 * 0 = never (the 128-row LDS-DMA kernel, as in a build with ESP_WGRAD_WS=0, where this call changes nothing).
 * Unsplit, both kernels give the same C bit for bit.  The same switch, with the same meaning, covers the fp32
 * RC x I2C_RC GEMM (the conv2 weight gradient, B gathered from the NHWC conv1 map on the producer waves) when C % 4
 * == 0, Bn * H * W < 2^24 and the map holds < 2^32 elements; esp_conv2_wgrad_bf16 is not affected.  Returns the
 * previous mode. */
int esp_set_wgrad_ws(int mode);
/* (An addition to ABI 42.)  The kernel of the unsplit fp32 KC x KC and I2C_KC x KC GEMMs on B planes (esp_gemm_f32_bp)
 * whose epilogue is bias + ReLU, or (KC x KC) bias + dropout + alpha + beta R -- the conv2 forward and the FFN w_2
 * forward -- of every later launch (process-wide): 1 (default) = the warp-specialised kernel (csrc/gemm_fwd_ws.hip:
 * 128 x 256 tiles, A gathered and split once per block on producer waves) for the shapes that measured faster
 * (N % 256 == 0, K >= 512, >= 4 rounds of 128-row tiles over the CUs); 2 = that kernel for every structurally
 * eligible launch (unbatched, unsplit, no row sums, wide epilogue; gathered A: C % 32 == 0, K % 32 == 0, Bn * H * W <
 * 2^24, the map < 2^32 elements); 0 = never (the LDS-DMA kernel, as in a build with ESP_FWD_WS=0, where this call
 * changes nothing).  Both kernels give the same C bit for bit.  Returns the previous mode. */
int esp_set_fwd_ws(int mode);
/* Launches of that kernel by this process so far (tests: which kernel a call took). */
long esp_get_fwd_ws_launches(void);
/* (An addition to ABI 42.)  The kernel of the conv2 input gradient's four parity-class GEMMs (esp_conv2_dgrad_bits,
 * esp_conv2_dgrad_c1fold) on the fp32 split path (fp32 dz2, fp32 compute type) of every later call (process-wide):
 * 1 (default) = the warp-specialised kernel (csrc/gemm_dgrad_ws.hip: 128 x 256 tiles, dz2 gathered and split once per
 * block on producer waves) for the classes that measured faster (by K = taps * D, see conv2_dgrad_impl) when the
 * class has >= 4 rounds of 128-row tiles over the CUs; 2 = that kernel for every structurally eligible class launch
 * (D % 256 == 0, D <= 512, B * Ha * We and B * T2 * F2 < 2^24, dz2 < 2^32 elements); 0 = never (the LDS-DMA kernel, as in a build with ESP_DGRAD_WS=0, where
 * this call changes nothing).  Both kernels give the same dz1 bit for bit; the folded dW / db differ in the order of
 * the per-block sums only.  esp_conv2_dgrad (fp32 mask map) and the bf16 forms are not affected.  Returns the previous
 * mode. */
int esp_set_dgrad_ws(int mode);
/* Launches of that kernel by this process so far: one per class GEMM it took (tests). */
long esp_get_dgrad_ws_launches(void);
/* esp_gemm_f32 with B also given as its three bf16 split planes (esp_f32_to_planes of the fp32 B,
 * b = hi + mid + lo exactly): the same fp32 split products as esp_gemm_f32 on the fp32 B, in the same
 * order, bit for bit (split-K counts may differ: a different tile width), without splitting B in the
 * GEMM's k-loop.  b_planes: plane 0; plane p at b_planes + p * b_pstride bf16 elements; ldbp, sbp1,
 * sbp2 in bf16 elements.  Used when the fp32 compute type is active, mode_b is KC or RC and the planes
 * qualify (16-B aligned, ldbp / strides / pstride % 8 == 0, K % 8 == 0 for KC, N % 8 == 0 for RC);
 * otherwise -- or when the epilogue kind has no B-planes kernel -- the fp32 B (which may then not
 * be NULL) is used.  Reference: every nn.Linear / Conv weight operand of the step (weights are
 * split once per step, kernels.py). */
int esp_gemm_f32_bp(int mode_a, int mode_b, int M, int N, int K, int batch, int nb2, const float* A, long lda,
                    long sa1, long sa2, const float* B, long ldb, long sb1, long sb2, float* C, long ldc,
                    long sc1, long sc2, const float* bias, float alpha, float beta, const float* R, int act,
                    float* aux, float drop_p, unsigned long long seed, int bwd_act, const float* pre, float* rowsum,
                    const int* im2col_a, float* work, long work_bytes, const void* b_planes, long ldbp, long sbp1,
                    long sbp2, long b_pstride, void* stream);
/* esp_gemm_f32 with either operand, or both, also given as its three bf16 split planes (layout of
 * esp_gemm_f32_bp's B planes; A planes: a_planes, ldap, sap1, sap2, a_pstride in bf16 elements, mode KC
 * or RC, K % 8 == 0 for KC, M % 8 == 0 for RC).  Both as planes: no operand split in the k-loop (the
 * same products, bit for bit; 64-wide tiles).  An operand whose planes do not qualify, or a launch
 * with no planes kernel, takes its fp32 values (which may then not be NULL); A NULL fp32 operand with
 * qualifying planes is allowed.  mode_a, mode_b: 0 (KC) or 1 (RC).
 * c_nplanes 3 or 1: C is written as bf16 planes (the exact split / bf16) instead of fp32 -- C points at
 * plane 0, plane p at C + p * c_pstride bf16 elements, ldc / sc1 / sc2 in bf16 elements (aux and pre
 * share those offsets in fp32 elements) -- for the epilogues whose result only GEMMs read: plain
 * (the attention context), bias + activation + dropout + derivative (the FFN hidden state) and the
 * backward multiply by pre (bwd_act ACT_MUL, no dropout / bias: the FFN hidden-state gradient);
 * N % 4 == 0, no residual, no row sums, never split-K.  0: fp32 C. */
int esp_gemm_f32_pl(int mode_a, int mode_b, int M, int N, int K, int batch, int nb2, const float* A, long lda,
                    long sa1, long sa2, const void* a_planes, long ldap, long sap1, long sap2, long a_pstride,
                    const float* B, long ldb, long sb1, long sb2, const void* b_planes, long ldbp, long sbp1,
                    long sbp2, long b_pstride, float* C, long ldc, long sc1, long sc2, const float* bias,
                    float alpha, float beta, const float* R, int act, float* aux, float drop_p,
                    unsigned long long seed, int bwd_act, const float* pre, float* rowsum, int c_nplanes,
                    long c_pstride, float* work, long work_bytes, void* stream);
/* The three bf16 planes of a rows x cols fp32 matrix x (row pitch ldx): plane p at y + p * pstride
 * (bf16 elements, row pitch ldy), hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to
 * nearest even with exact fp32 residuals, so x = hi + mid + lo for every finite x.  Columns
 * cols..ldy-1 are written 0.  ldy, pstride % 8 == 0, pstride >= rows * ldy, y 16-B aligned. */
int esp_f32_to_planes(const float* x, void* y, long rows, int cols, long ldx, long ldy, long pstride, void* stream);
/* bf16-operand GEMM (the C5 reduced-precision path): A and B bf16 (bits of __bf16 /
 * torch.bfloat16) in mode KC or RC as esp_gemm_f32 (KC: [rows][K]; RC: [K][rows], staged for
 * transposing LDS reads), fp32 accumulate; C, the epilogue (bias, act, aux, dropout, bwd_act /
 * pre, residual) and split-K exactly as esp_gemm_f32.  K, lda, ldb and the batch strides in bf16
 * elements, multiples of 8; A, B 16-B aligned; an RC operand's row count a multiple of 8.
 * rowsum != NULL (mode_a RC, batch 1): rowsum[m] += sum_k A(m,k) in fp32 over the bf16 values.  The
 * operands come from esp_f32_to_bf16 (activations, gradients) or bf16 weight copies. */
int esp_gemm_bf16(int mode_a, int mode_b, int M, int N, int K, int batch, int nb2, const void* A, long lda,
                  long sa1, long sa2, const void* B, long ldb, long sb1, long sb2, float* C, long ldc,
                  long sc1, long sc2, const float* bias, float alpha, float beta, const float* R, int act,
                  float* aux, float drop_p, unsigned long long seed, int bwd_act, const float* pre, float* rowsum,
                  float* work, long work_bytes, void* stream);
/* esp_gemm_bf16 with C written as its bf16 plane (c_nplanes 1: hi = bf16(C), the reduced-precision
 * path's GEMM-only activations and gradients) under the rules of esp_gemm_f32_pl's c_nplanes: the
 * plain, FFN w_1 and ACT_MUL epilogues, N % 4 == 0, no residual / row sums, never split-K. */
/* The bf16 mode's conv2 forward (subsampling.py:53-87, NHWC): z2 = ReLU(im2col(z1_16) w16^T + bias) on
 * bf16 operands (z1_16 from esp_conv1_fwd_bf16, w16 the (o, kt, kf, c)-laid weights in bf16, row pitch
 * 9D), fp32 accumulate and output.  D % 64 == 0, 16-B aligned operands. */
int esp_conv2_fwd_bf16(const void* z1_16, const void* w16, const float* bias, float* z2, int B, int T1, int F1, int D,
                       float* work, long work_bytes, void* stream);
/* The bf16 mode's conv2 weight gradient: dw (D x 9D, (o, kt, kf, c) order) = dz2^T im2col(z1) and
 * db += column sums of dz2, on bf16 operands (dz2_16 [pixels][D], z1_16 from esp_conv1_fwd_bf16); an
 * even pixel count, D % 64 == 0, 16-B aligned; `work` the split-K partials as esp_gemm_f32's. */
int esp_conv2_wgrad_bf16(const void* dz2_16, const void* z1_16, float* dw, float* db, int B, int T1, int F1, int D,
                         float* work, long work_bytes, void* stream);
/* esp_conv2_dgrad with dz2 in bf16 (the bf16 mode): the class GEMMs on bf16 operands (workspace as
 * esp_conv2_dgrad's).  D % 64 == 0. */
int esp_conv2_dgrad_bf16(const void* dz2_16, const float* W, const float* z1, float* dz1, int B, int T1, int F1, int D,
                         const float* zeros16, float* wc_work, long work_bytes, void* stream);
int esp_gemm_bf16_pl(int mode_a, int mode_b, int M, int N, int K, int batch, int nb2, const void* A, long lda,
                     long sa1, long sa2, const void* B, long ldb, long sb1, long sb2, void* C, long ldc,
                     long sc1, long sc2, const float* bias, float alpha, float beta, int act, float* aux,
                     float drop_p, unsigned long long seed, int bwd_act, const float* pre, int c_nplanes,
                     long c_pstride, float* work, long work_bytes, void* stream);
/* y = bf16(x) (round to nearest even) for a rows x cols fp32 matrix (row pitch ldx); transpose:
 * y[c * ldy + r] (a cols x rows bf16 matrix), else y[r * ldy + c]. */
int esp_f32_to_bf16(const float* x, void* y, long rows, int cols, long ldx, long ldy, int transpose,
                    void* stream);

/* ---- element-wise (positionwise_feed_forward.py:32, conformer/swish.py:13-18, dropout) */
int esp_act_bwd(const float* dy, const float* h, float* dx, long n, int act, float drop_p,
                unsigned long long seed, long idx_off, void* stream);
int esp_scale_dropout(const float* x, float* y, long n, float alpha, float drop_p,
                      unsigned long long seed, const float* r, float beta, void* stream);
/* y = alpha * drop(x) written as bf16 planes (nplanes 3 exact split, 1 bf16; plane p at y + p * pstride
 * bf16 elements) of a matrix with ld == cols (n = rows * cols, % 4 == 0): the same masks as
 * esp_scale_dropout for the same (drop_p, seed). */
int esp_scale_dropout_planes(const float* x, void* y, long n, long pstride, int nplanes, float alpha, float drop_p,
                             unsigned long long seed, void* stream);
int esp_scale_by_dev(float* x, long n, const float* s, void* stream);
/* decoder embedding + abs positional encoding (transformer_decoder.py:68-71, embedding.py:81-94) */
int esp_embed_fwd(const long long* tok, const float* E, const float* pe, float* y, int nrows, int L,
                  int D, float xscale, float drop_p, unsigned long long seed, void* stream);
int esp_embed_bwd(const long long* tok, const float* dy, float* dE, int nrows, int V, int D,
                  float xscale, float drop_p, unsigned long long seed, void* stream);
/* SpecAug with injected draws (specaug.py:89-96, time_warp.py:9-88, mask_along_axis.py:8-68):
 * lens (B) int32; warp (B,2) {center, warped} or NULL (center<=0: no warp for that row);
 * fmask (B,nf,2) / tmask (B,nt,2) {pos, width}. */
int esp_specaug(const float* x, float* y, int B, int T, int F, const int* lens, const int* warp,
                const int* fmask, int nf, const int* tmask, int nt, void* stream);
/* UtteranceMVN(norm_means=True, norm_vars=False), in place (utterance_mvn.py:45-80) */
int esp_utterance_mvn(float* x, int B, int T, int F, const int* lens, void* stream);
/* clip_grad_norm_ + Adam over flat buffers (trainer.py:642-686, abs_task.py:78-79) */
int esp_grad_norm(const float* g, long n, float max_norm, double* work, long work_bytes, float* out3,
                  void* stream);
int esp_adam(float* p, const float* g, float* m, float* v, long n, const float* clip3, float lr,
             double b1, double b2, float eps, float wd, int step, void* stream);
/* Device-resident optimizer bookkeeping (a whole training step as one HIP graph):
 * state (2 doubles) = {Adam steps applied, WarmupLR steps taken}.  esp_opt_hyper writes the
 * next step's {lr, 1-b1^t, sqrt(1-b2^t)} (warmuplr.py:43-50, torch Adam) to hyper (3 floats);
 * esp_adam_dev reads them; esp_opt_advance counts the step only if clip3[2] (finite) != 0,
 * which is exactly when trainer.py:651-686 steps the optimizer and the scheduler. */
int esp_opt_hyper(const double* state, double base_lr, double warmup, double b1, double b2, float* hyper,
                  void* stream);
int esp_adam_dev(float* p, const float* g, float* m, float* v, long n, const float* clip3,
                 const float* hyper, double b1, double b2, float eps, float wd, void* stream);
int esp_opt_advance(double* state, const float* clip3, void* stream);
/* ABI 30: torch.optim.Adam(amsgrad=True) (the optim_conf key abs_task.py:856-880 passes through): as
 * esp_adam / esp_adam_dev, the denominator on vmax = max(vmax, exp_avg_sq), kept in place (n floats).
 * ABI 30 also passes beta1 / beta2 of every Adam entry as double: 1 - beta and the bias corrections are
 * formed in double as torch forms them from python floats (fp32 1 - 0.999f is 1.3e-5 off 0.001). */
int esp_adam_amsgrad(float* p, const float* g, float* m, float* v, float* vmax, long n, const float* clip3,
                     float lr, double b1, double b2, float eps, float wd, int step, void* stream);
int esp_adam_dev_amsgrad(float* p, const float* g, float* m, float* v, float* vmax, long n, const float* clip3,
                         const float* hyper, double b1, double b2, float eps, float wd, void* stream);
/* Dropout key: every dropout kernel XORs its seed with *key when set (NULL: off).  The key
 * lives in device memory so a replayed HIP graph draws fresh masks; esp_rng_advance mixes it
 * (splitmix64) on device. */
int esp_set_rng_key(const unsigned long long* key);
int esp_rng_advance(unsigned long long* key, void* stream);

/* ---- normalisation (layer_norm.py:12-38; convolution.py:56-79) */
int esp_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* mean,
                      float* rstd, int M, int D, float eps, void* stream);
/* esp_layernorm_fwd with y written as bf16 planes for GEMM readers (kernels.Planes): nplanes 3 = the
 * exact split hi + mid + lo (esp_f32_to_planes), 1 = bf16(y); plane p at y + p * pstride (bf16
 * elements), row pitch ldy (>= D, % 4 == 0).  D % 4 == 0, x / w / b 16-B aligned, y 8-B aligned. */
int esp_layernorm_fwd_planes(const float* x, const float* w, const float* b, void* y, long ldy, long pstride,
                             int nplanes, float* mean, float* rstd, int M, int D, float eps, void* stream);
/* ABI 29: y written in fp32 (yf, row pitch D, 16-B aligned) AND as planes (as esp_layernorm_fwd_planes):
 * the fp32 mode's LayerNorm outputs that feed a Linear's forward (fp32 A) and its weight gradient (the
 * planes as B, gemm_kernels.h PREC 3).  Replaces the same LayerNorm as esp_layernorm_fwd (layer_norm.py:12-38). */
int esp_layernorm_fwd_dual(const float* x, const float* w, const float* b, float* yf, void* y, long ldy,
                           long pstride, int nplanes, float* mean, float* rstd, int M, int D, float eps,
                           void* stream);
int esp_layernorm_bwd(const float* dy, const float* x, const float* w, const float* mean,
                      const float* rstd, float* dx, int accumulate, float* dw, float* db, int M,
                      int D, float* work, long work_bytes, void* stream);
int esp_colsum(const float* x, int M, int N, long ld, float* out, int accumulate, float* work,
               long work_bytes, void* stream);
int esp_glu_fwd(const float* u, float* g, long rows, int D, void* stream);
int esp_glu_bwd(const float* u, const float* dg, float* du, long rows, int D, void* stream);
/* esp_glu_bwd with du written as bf16 planes (nplanes 3 exact split, 1 bf16; row pitch 2D, plane p at
 * du + p * pstride bf16 elements) for pointwise_conv1's gradient GEMMs; D % 4 == 0. */
int esp_glu_bwd_planes(const float* u, const float* dg, void* du, long pstride, int nplanes, long rows, int D,
                       void* stream);
/* tvalid (device int, nullable): the batch is padded to T frames per utterance but only the
 * first *tvalid exist in the reference batch (length-bucketed HIP graphs).  The depthwise
 * convolution reads frames >= *tvalid as its zero padding and writes 0 there; BatchNorm
 * statistics count B * (*tvalid) rows and the excluded rows get a zero gradient.  With tvalid,
 * M = B * T rows for the BatchNorm calls.  BatchNorm workspaces: D * 1536 (forward) and
 * 2 * D * 1536 (backward) doubles — the statistics are reduced in at most 1536 row chunks. */
int esp_dwconv1d(const float* x, const float* W, const float* bias, float* y, int Bn, int T, int D,
                 int K, int flip, const int* tvalid, void* stream);
int esp_dwconv1d_wgrad(const float* dy, const float* x, float* dW, int Bn, int T, int D, int K,
                       float* work, long work_bytes, const int* tvalid, void* stream);
/* ABI 33: the Branchformer cgMLP's convolutional spatial gating unit (cgmlp.py:15-81; gate_activation identity,
 * no linear after the convolution).  v (B*T, 2C) is channel_proj1's plain output, GELU (erf form) is applied on
 * load: a_r = GELU(v[:, :C]), a_g = GELU(v[:, C:]), n = LayerNorm_C(a_g) (gamma, beta, eps), g = dwconv_k(n) + bias
 * over each utterance's own T rows (zero outside [0, T) and at or after *tvalid; no length mask: padded frames
 * of a short utterance are read like any other), o = drop(a_r * g) with the esp_scale_dropout index r*C + c.
 * C % 4 == 0, k odd and <= 63, 16-B aligned tensors.  Rows at or after *tvalid are written as 0.
 *   esp_csgu_stats: mean / rstd (M) of a_g per row.
 *   esp_csgu_fwd: o (B*T, C); neither a nor n is written.
 *   esp_csgu_bwd_gate: from dout = dL/do: dv[:, :C] = drop'(dout) g GELU'(v_r), dg = drop'(dout) a_r (B*T, C)
 *     and n (B*T, C).  dv (B*T, 2C) is fp32 (nplanes 0) or bf16 planes (nplanes 1 / 3, plane p at dv + p * pstride
 *     bf16 elements, row pitch 2C).
 *   esp_csgu_bwd_norm: from dn = dL/dn: dv[:, C:] = LN'(dn) GELU'(v_g) and pxh = dn * xhat (B*T, C), whose column
 *     sum is the LayerNorm weight gradient (dn's is the bias gradient).
 * Between the two backward calls: dn = esp_dwconv1d(dg, flip), esp_dwconv1d_wgrad(dg, n), esp_colsum(dg). */
/* The E-Branchformer's enhanced merge around merge_proj (csrc/ebf_merge.hip; e_branchformer_encoder.py:158-163; a
 * pure addition to the ABI above).  xc (B*T, C) is the concatenation [x1, x2] of the two branch outputs (C = 2D), W (C, k)
 * and bias (C) are depthwise_conv_fusion's:
 *   u[b,t,c] = xc[b,t,c] + bias[c] + sum_j W[c,j] xc[b, t + j - (k-1)/2, c]
 * over each utterance's own T rows (zero outside [0, T) and at or after *tvalid; no length mask: padded frames of a
 * short utterance are read like any other).  Rows at or after *tvalid are written as 0.  C % 8 == 0, k odd and
 * <= 31, any T >= 1, 16-B aligned tensors; other arguments fail with status -1.
 *   esp_ebf_merge_fwd: u (B*T, C), fp32 (nplanes 0) or bf16 planes (nplanes 1 / 3, plane p at u + p * pstride bf16
 *     elements, row pitch C): merge_proj's operand format.
 *   esp_ebf_merge_bwd: from du = dL/du (B*T, C; rows at or after *tvalid are not read): the input gradient
 *     du + conv^T(du) as its two contiguous (B*T, C/2) halves d1 | d2, and dW (C, k) += sum du[b,t,c] xc[b,t+j-pad,c],
 *     dbias (C) += sum du[b,t,c].  The sums are formed per block in the workspace
 *     (esp_ebf_merge_bwd_workspace_bytes) and added in a fixed order by a second kernel (no atomics: repeated
 *     launches give the same bits). */
int esp_ebf_merge_fwd(const float* xc, const float* W, const float* bias, void* u, long pstride, int nplanes, int B,
                      int T, int C, int k, const int* tvalid, void* stream);
int esp_ebf_merge_bwd(const float* du, const float* xc, const float* W, float* d1, float* d2, float* dW, float* dbias,
                      int B, int T, int C, int k, float* work, long work_bytes, const int* tvalid, void* stream);
int esp_csgu_stats(const float* v, long M, int C, float eps, float* mean, float* rstd, void* stream);
int esp_csgu_fwd(const float* v, const float* mean, const float* rstd, const float* gamma, const float* beta,
                 const float* W, const float* bias, float* o, int B, int T, int C, int k, float drop_p,
                 unsigned long long seed, const int* tvalid, void* stream);
int esp_csgu_bwd_gate(const float* v, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      const float* W, const float* bias, const float* dout, void* dv, long pstride, int nplanes,
                      float* dg, float* n, int B, int T, int C, int k, float drop_p, unsigned long long seed,
                      const int* tvalid, void* stream);
int esp_csgu_bwd_norm(const float* v, const float* mean, const float* rstd, const float* gamma, const float* dn,
                      void* dv, long pstride, int nplanes, float* pxh, int B, int T, int C, const int* tvalid,
                      void* stream);
int esp_bn_swish_fwd(const float* y, const float* gamma, const float* beta, float* s, float* mean,
                     float* rstd, float* run_mean, float* run_var, float momentum, float eps, int M,
                     int D, double* work, long work_bytes, int T, const int* tvalid, void* stream);
/* esp_bn_swish_fwd with s written as bf16 planes for pointwise_conv2, its only reader (nplanes 3:
 * the exact split, 1: bf16; plane p at s_planes + p * pstride bf16 elements, row pitch lds).
 * D, lds, pstride % 4 == 0; 16-B aligned y / gamma / beta, 8-B aligned planes. */
int esp_bn_swish_fwd_planes(const float* y, const float* gamma, const float* beta, void* s_planes, long lds,
                            long pstride, int nplanes, float* mean, float* rstd, float* run_mean, float* run_var,
                            float momentum, float eps, int M, int D, double* work, long work_bytes, int T,
                            const int* tvalid, void* stream);
/* eval mode: statistics from run_mean / run_var (mean / rstd written for inspection) */
int esp_bn_swish_eval(const float* y, const float* gamma, const float* beta, float* s, const float* run_mean,
                      const float* run_var, float eps, int M, int D, float* mean, float* rstd, void* stream);
int esp_bn_swish_bwd(const float* ds, const float* y, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta,
                     int M, int D, double* work, long work_bytes, float* sums, int T, const int* tvalid,
                     void* stream);

/* ---- attention glue (attention.py:64-96,145-165,240-263) */
int esp_heads_split(const float* src, long ld, int col0, int B, int T, int H, int dk,
                    const float* bias, float* dst, void* stream);
/* both head-major splits of esp_heads_split in one pass: dst_a = q + bias_a, dst_b = q + bias_b
 * (q + pos_bias_u, q + pos_bias_v; attention.py:240-250).  16-B aligned, dk, ld, col0 % 4 == 0. */
int esp_heads_split2(const float* src, long ld, int col0, int B, int T, int H, int dk, const float* bias_a,
                     float* dst_a, const float* bias_b, float* dst_b, void* stream);
int esp_add2d(const float* x, long ldx, float* y, long ldy, int M, int N, void* stream);
/* score rows (ac / attn / pdrop / dP / dS) have pitch lds >= Tk, bd / dbd rows pitch ldp >= P
 * (multiples of 4 keep every row 16-B aligned for the GEMMs' LDS-DMA staging); dropout
 * masks are keyed by the logical index row*Tk + j, independent of the pitch. */
int esp_attn_softmax_fwd(const float* ac, const float* bd, int relpos, int P, float sqrt_dk,
                         const int* klen, int nb, int causal, float* attn, float* pdrop,
                         float drop_p, unsigned long long seed, int Z, int Tq, int Tk, long lds,
                         long ldp, const int* tvalid, void* stream);  /* tvalid: legacy length bucket, see below */
int esp_attn_softmax_bwd(const float* attn, const float* dP, float* dS, float drop_p,
                         unsigned long long seed, float sqrt_dk, long rows, int Tk, long lds,
                         void* stream);
int esp_relshift_bwd(const float* dS, long lds, float* dbd, long ldp, int relpos, int Z, int T, int P,
                     void* stream);
/* esp_attn_softmax_bwd fused with esp_relshift_bwd (relpos 1 latest: P = 2T-1 columns; relpos 2
 * legacy: P = T columns): writes dS and every dbd element of the rows (pitch ldp) in one pass.
 * rows = Z*T. */
int esp_attn_softmax_bwd_relpos(const float* attn, const float* dP, float* dS, float* dbd, long ldp,
                                int relpos, float drop_p, unsigned long long seed, float sqrt_dk,
                                long rows, int T, long lds, const int* tvalid, void* stream);
/* ABI 29: the latest rel_shift's q_v gradient through the band scores, dq_v[z] = dbd[z] . p_h (z = h*nb + b):
 * the dbd.p contraction with each 128-row tile's k-loop over its rows' band union only (row i of dbd is 0
 * outside columns T-1-i .. 2T-2-i).  dbd (nb*H*T rows, pitch ldp >= 2T-1, % 4 == 0), p (2T-1 rows, pitch
 * ldpm, head h at column 64 h), out rows b*T + i (pitch ldo, head h at column 64 h); d_k = 64. */
int esp_relpos_dqv(const float* dbd, long ldp, const float* p, long ldpm, float* out, long ldo, int nb, int H,
                   int T, float* work, long work_bytes, void* stream);
/* ABI 29: the latest form (P = 2T-1) writing only row i's band of dbd, columns T-1-i .. 2T-2-i, into a
 * buffer whose other elements are already 0 (kept and zeroed once by the caller: nothing else writes it);
 * half the dbd bytes of esp_attn_softmax_bwd_relpos.  lds % 4 == 0, attn / dP / dS 16-B aligned. */
int esp_attn_softmax_bwd_relpos_band(const float* attn, const float* dP, float* dS, float* dbd, long ldp,
                                     float drop_p, unsigned long long seed, float sqrt_dk, long rows, int T,
                                     long lds, void* stream);
/* Fused latest rel-pos attention backward: dP = dctx V^T on the MFMA per 32-row block, attention
 * dropout adjoint, softmax adjoint, rel_shift adjoint -> dS (pitch lds) and dbd (pitch ldp).
 * dctx rows at dctx + (b*T+i)*ldd + 64h, V rows at vmat + (b*T+j)*ldv + 64h; d_k = 64, T <= 512. */
int esp_relpos_attn_bwd(const float* dctx, long ldd, const float* vmat, long ldv, const float* attn,
                        float* dS, float* dbd, long ldp, int nb, int H, float sqrt_dk, float drop_p,
                        unsigned long long seed, int T, long lds, void* stream);
/* Flash-style rel-pos self-attention (csrc/flash_relpos.hip), replacing attention.py:64-96 with
 * the latest (rel = 1, attention.py:240-263, P = 2T-1 position rows) or legacy (rel = 2,
 * attention.py:145-165 rel_shift, P = T rows) score assembly; d_k = 64, T <= 512.
 * q_u = q + pos_bias_u, q_v = q + pos_bias_v: (Z, T, 64) head-major, z = h*nb + b.  k / v rows at
 * kmat + (b*T + j)*ldk + 64h (vmat / ldv alike), p rows at p + row*ldp_row + 64h.
 * Forward: ctx (rows b*T + i, pitch ldc, head slice 64h) = dropout(softmax(s)) v, and the row
 * statistics stats (Z, T, 2) = {max, 1/sum} the backward recomputes P from.  No (Z,T,T) tensor. */
int esp_relpos_flash_fwd(const float* qu, const float* qv, const float* kmat, long ldk, const float* vmat,
                         long ldv, const float* p, long ldp_row, int rel, int nb, int H, float sqrt_dk,
                         const int* klen, float* ctx, long ldc, float* stats, float drop_p,
                         unsigned long long seed, int T, void* stream);
/* Backward of esp_relpos_flash_fwd: recomputes the scores, writes dq (= dq_u + dq_v, rows b*T + i,
 * pitch ldq, head slice 64h; overwritten), dS = dL/d(ac + bd) and the dropped probabilities
 * pdrop (Z, T, lds) for the key-side GEMMs dK = dS^T q_u and dV = pdrop^T dctx, the per-block
 * pos_bias column sums bias_part (Z, ceil(T/32), 2, 64) and, for legacy, carry (Z, ceil(T/32), 64).
 * ctx / dctx: the forward output and its gradient (pitch ldc). */
int esp_relpos_flash_bwd(const float* qu, const float* qv, const float* kmat, long ldk, const float* vmat,
                         long ldv, const float* p, long ldp_row, int rel, int nb, int H, float sqrt_dk,
                         const int* klen, const float* ctx, const float* dctx, long ldc, const float* stats,
                         float drop_p, unsigned long long seed, int T, float* dq, long ldq, float* dS,
                         float* pdrop, long lds, float* bias_part, float* carry, void* stream);
/* linear_pos gradient input from dS and q_v: dp (P x 64H, pitch ldp; overwritten) =
 * sum_{b,i} dbd^T q_v with the rel_shift adjoint read along the diagonals of dS (no dbd tensor);
 * pos_bias_u / pos_bias_v gradients += the column sums of esp_relpos_flash_bwd (du, dv: H x 64);
 * legacy: adds each block's carry to dq (pitch ldq).  work: >= H * ceil(nb/8) * (2T-1) * 64 floats. */
int esp_relpos_dp(const float* dS, long lds, const float* qv, int rel, int nb, int H, int T, float* dp, long ldp,
                  const float* bias_part, const float* carry, float* du, float* dv, float* dq, long ldq,
                  float* work, long work_floats, void* stream);
/* ABI 34: the query gradient of latest rel-pos attention straight from dS (csrc/attention_bwd.hip; d_k = 64,
 * T <= 480): dq (rows b*T + i, pitch ldq, head h at column 64 h; overwritten) = dS k + Dbd p, the rel_shift
 * adjoint Dbd[i][T-1-i+j] = dS[i][j] read from the staged dS rows with a per-row skew (no dbd tensor), on the
 * GEMMs' six bf16 split products.  dS: nb*H*T rows of pitch lds (% 4 == 0, 16-B aligned), z = h*nb + b; k rows
 * at kmat + (b*T + j)*ldk + 64 h; p: 2T-1 rows of pitch ldpm, head h at column 64 h.  bias_part
 * (nb*H, ceil(T/32), 2, 64): per-block column sums of dq_u and dq_v, which esp_relpos_dp reduces in fixed order
 * into the pos_bias_u / pos_bias_v gradients. */
int esp_relpos_dq(const float* dS, long lds, const float* kmat, long ldk, const float* p, long ldpm, float* dq,
                  long ldq, float* bias_part, int nb, int H, int T, void* stream);
/* Fully fused latest rel-pos attention probabilities (attention.py:240-263 with the latest rel_shift,
 * embedding.py:173-244; 64-96): ac = (q+u) k^T AND the bd band bd_shift[i][j] = q_v[i] . p[j + T-1-i] on the
 * MFMA per 32-row block, then s = (ac + bd_shift)/sqrt(dk), key mask j < klen[b], softmax, dropout copy: no
 * score tensor other than attn / pdrop reaches HBM.  q_u, q_v (Z,T,64) head-major z = h*nb + b; k row j of
 * utterance b, head h at kmat + (b*T + j)*ldk + 64h (the fused qkv projection); p: P = 2T-1 rows of pitch
 * ldp_row, head h at column 64h.  d_k must be 64; T such that the 32 x (32*ceil((T+31)/32)+4) float window
 * (+ 256 floats of row partials) fits 64 KB (T <= 449).
 * ABI 37: esp_relpos_softmax_fwd (the same band window over an ac tensor from HBM; no caller since the fused
 * forms) is removed. */
int esp_relpos_attn_fwd(const float* qu, const float* qv, const float* kmat, long ldk, const float* p,
                        long ldp_row, int nb, int H, float sqrt_dk, const int* klen, float* attn,
                        float* pdrop, float drop_p, unsigned long long seed, int T, long lds,
                        void* stream);
/* Rel-pos attention backward without the (Z,T,T) dP tensor (FlashAttention-2's row term):
 * esp_attn_bwd_prep: dot[z*T+i] = dctx_i . ctx_i per head (= sum_j P_drop[i][j] dP[i][j]) and
 * the bd-gradient elements without a rel_shift source zeroed; esp_attn_dscores: dP = dctx V^T
 * on the MFMA with dS = P (drop'(dP) - dot) / sqrt(d_k) -> dS (pitch lds) and its latest / legacy
 * rel_shift adjoint -> dbd (pitch ldp) in the epilogue.  Layouts as esp_relpos_attn_probs (dctx,
 * ctx (B*T, H*dk) rows of pitch ldd / ldc; V rows at vmat + (b*T + j)*ldv + h*dk; attn / dS
 * (Z,T) rows of pitch lds, 16-B aligned).  Replaces the dP GEMM + esp_attn_softmax_bwd_relpos
 * (attention.py:64-96, 145-165 backward). */
/* ABI 34: dbd NULL in both: the row dots alone / dS alone (no rel_shift adjoint scatter), for the backward
 * that reads dS directly (esp_relpos_dq, esp_relpos_dp). */
int esp_attn_bwd_prep(const float* dctx, long ldd, const float* ctx, long ldc, int nb, int H, int dk, int T,
                      float* dot, float* dbd, long ldp, int relpos, void* stream);
int esp_attn_dscores(const float* dctx, long ldd, const float* vmat, long ldv, const float* attn, const float* dot,
                     float* dS, float* dbd, long ldp, int relpos, int nb, int H, int dk, float sqrt_dk,
                     float drop_p, unsigned long long seed, int T, long lds, void* stream);
/* Rel-pos attention probabilities for latest (relpos 1: p has P = 2T-1 rows) AND legacy
 * (relpos 2: p has P = T rows, legacy rel_shift attention.py:145-165) rel_shift, one wave per
 * 16 query rows with every score row in registers (no block synchronisation): ac and the bd band
 * on v_mfma_f32_16x16x4_f32, rel_shift through a per-wave LDS ring, key mask, softmax, dropout
 * copy.  Operands as esp_relpos_attn_fwd; d_k = 64, T <= 512; attn / pdrop 16-B aligned with
 * lds % 4 == 0 (columns T .. round_up(T, 4) - 1 of the pitch are written as 0).  Replaces, for these shapes, the
 * reference's matrix_ac / matrix_bd matmuls + rel_shift + softmax + dropout
 * (attention.py:240-263, 64-96). */
/* ABI 31: the relpos_probs_lds_kernel LDS slot-schedule check (attention.hip; a debug build, make
 * VARIANT=_slotchk EXTRA=-DESP_ATTN_SLOT_CHECK=1): slot-generation mismatches counted since the last call
 * (the count is reset), -1 in a build without the check. */
int esp_attn_slot_check_errors(void);
int esp_relpos_attn_probs(const float* qu, const float* qv, const float* kmat, long ldk, const float* p,
                          long ldp_row, int relpos, int nb, int H, float sqrt_dk, const int* klen,
                          float* attn, float* pdrop, float drop_p, unsigned long long seed, int T,
                          long lds, const int* tvalid, void* stream);
/* tvalid (esp_relpos_attn_probs, esp_attn_softmax_bwd_relpos; legacy only, may be NULL): device int
 * T' <= T when the batch is a length bucket padded from T' to T frames.  The legacy rel_shift then
 * uses the reference batch's table positions j + T'-1-i (they depend on T'; the latest ones, i - j,
 * do not), and the adjoint writes the unpadded dbd zero-extended (rows and columns >= T' are 0). */

/* ---- feature front end: DefaultFrontend + GlobalMVN
 * esp_fbank_fwd: STFT (center, reflect, window of length n_fft, onesided) -> power -> mel
 * (dense (n_fft/2+1, n_mels) matrix, band [mel_lo[m], mel_hi[m]) nonzero) -> clamp 1e-10 ->
 * log; frames t >= lens[b]/hop + 1 written as 0 (default.py:82-131, stft.py:63-160,
 * log_mel.py:57-81).  wave (B, N) row pitch ldw; lens (device int32, samples); twiddle
 * n_fft (cos, -sin) pairs of exp(-2 pi i j / n_fft); out (B, T, n_mels), T = N/hop + 1.
 * n_fft even in [16, 2048]: radix-2 FFT when a power of two, direct DFT otherwise.
 * nvalid (may be NULL): device int N' <= N, the reference batch's sample count when the batch is
 * padded to a length bucket: the centre padding reflects at N' (frames >= N'/hop + 1 are 0). */
int esp_fbank_fwd(const float* wave, long ldw, const int* lens, int B, int N, int n_fft, int hop,
                  const float* window, const float* twiddle, const float* melw, const int* mel_lo,
                  const int* mel_hi, int n_mels, float* out, int T, const int* nvalid, void* stream);
/* GlobalMVN in place: x (B,T,F) -> ((x - mean), frames t >= lens[b] zeroed) / std
 * (global_mvn.py:67-90). */
int esp_global_mvn(float* x, const int* lens, int B, int T, int F, const float* mean,
                   const float* stdv, int norm_means, int norm_vars, void* stream);

/* ---- Conv2dSubsampling (subsampling.py:53-87), NHWC */
int esp_conv1_fwd(const float* x, const float* W, const float* bias, float* z, int B, int T,
                  int F, int D, void* stream);
/* esp_conv1_fwd writing z's bf16 copy (RNE) to z16 too (8-B aligned): the bf16 mode's conv2 operand. */
int esp_conv1_fwd_bf16(const float* x, const float* W, const float* bias, float* z, void* z16, int B, int T, int F,
                       int D, void* stream);
/* ABI 32: esp_conv1_fwd (z16 optional, as esp_conv1_fwd_bf16) also writing the ReLU mask as a packed bit map:
 * bit c % 32 of zbits[p * D/32 + c / 32] = (z[p][c] > 0), D % 32 == 0, 4-B aligned (replaces the fp32 map
 * as the conv2 input gradient's mask operand: esp_conv2_dgrad_bits reads 1/32 of the bytes). */
int esp_conv1_fwd_bits(const float* x, const float* W, const float* bias, float* z, void* z16, unsigned* zbits, int B,
                       int T, int F, int D, void* stream);
/* conv2 input gradient as 4 implicit GEMMs (one per parity class of the conv1 output grid):
 * dz1 = relu'(z1) * conv_transpose(dz2, W), W = Conv2d(D,D,3,2).weight (o,c,kt,kf) as the
 * reference stores it; no 9x column buffer.  zeros16: >= 16 B of zeros (device); wc_work:
 * 9*D*D floats (the per-class weight re-layout).  D % 32 == 0. */
int esp_conv2_dgrad(const float* dz2, const float* W, const float* z1, float* dz1, int B, int T1, int F1,
                    int D, const float* zeros16, float* wc_work, long work_bytes, void* stream);
/* ABI 32: esp_conv2_dgrad / esp_conv2_dgrad_bf16 with the conv1 ReLU mask from esp_conv1_fwd_bits' bit map
 * (z1bits) instead of the fp32 map; exactly one of dz2 (fp32) / dz2_16 (bf16, D % 64 == 0) non-NULL. */
int esp_conv2_dgrad_bits(const float* dz2, const void* dz2_16, const float* W, const unsigned* z1bits, float* dz1,
                         int B, int T1, int F1, int D, const float* zeros16, float* wc_work, long work_bytes,
                         void* stream);
/* ABI 32: esp_conv2_dgrad_bits with conv1's weight / bias gradient folded into the class GEMMs' epilogue
 * (replaces esp_conv2_dgrad_bits + esp_conv1_wgrad, subsampling.py:53-87 backward): dW (D x 9) += sum over the
 * conv1 map of dz1 * x-patch, db (D) += sum of dz1, dz1 never materialised.  x: the conv1 input (B, T, F) as
 * esp_conv1_fwd took it; c1_work: esp_conv2_c1fold_workspace_bytes() (per-block partial records + their
 * fixed-order reduction: deterministic).  D % 128 == 0, D <= 512. */
int esp_conv2_dgrad_c1fold(const float* dz2, const void* dz2_16, const float* W, const unsigned* z1bits,
                           const float* x, int T, int F, float* dW, float* db, int B, int T1, int F1, int D,
                           const float* zeros16, float* wc_work, long work_bytes, float* c1_work,
                           long c1_work_bytes, void* stream);
long esp_conv2_c1fold_workspace_bytes(void);
int esp_col2im_relu(const float* dcol, const float* z1, float* dz1, int B, int T1, int F1, int D,
                    void* stream);
int esp_conv1_wgrad(const float* x, const float* dz1, float* dW, float* db, int B, int T, int F,
                    int D, float* work, long work_bytes, void* stream);
/* ABI 31: input_layer "conv2d6" (espnet/nets/pytorch_backend/transformer/subsampling.py:101-146
 * Conv2dSubsampling6: its second Conv2d(D, D, 5, 3)) on explicit columns.  NHWC x [B, T1, F1, C] ->
 * col [B*T2*F2, k*k*C] with row p = (b, t2, f2), column (kt*k + kf)*C + c, T2 = (T1-k)/s + 1,
 * F2 = (F1-k)/s + 1 (a KC x KC GEMM with the (o, kt, kf, c) weight is then the convolution);
 * col2im_relu_nhwc: dx = relu'(z) * the column adjoint (taps summed kt, kf ascending).  C % 4 == 0. */
int esp_im2col_nhwc(const float* x, float* col, int B, int T1, int F1, int C, int k, int s, void* stream);
int esp_col2im_relu_nhwc(const float* dcol, const float* z, float* dx, int B, int T1, int F1, int C, int k,
                         int s, void* stream);
int esp_permute3(const float* in, float* out, int O, int Bd, int Ad, int accumulate, void* stream);

/* ---- losses (ctc.py:39-97, label_smoothing_loss.py:41-63, nets_utils.py:299-320,
 *      espnet/nets/pytorch_backend/ctc.py:185-249) */
int esp_log_softmax(const float* x, float* y, long rows, int V, void* stream);
/* Loss internals run in fp64 where fp32 rounding would exceed the 1e-4 loss gate: the CTC
 * alpha/beta recursions (values ~ -10^3), per-utterance nll, per-row label-smoothing KL and
 * the final reductions.  nll (B) and row_loss (R) are fp64; work >= 2*B*T*(2*Umax+1) doubles. */
int esp_ctc_loss(const float* lp, const long long* labels, int Umax, const int* ilen,
                 const int* tlen, int B, int T, int V, int blank, float gscale, int zero_infinity,
                 double* nll, float* grad, double* work, long work_bytes, void* stream);
int esp_label_smoothing(const float* x, const long long* target, long rows, int V, int ignore,
                        float smoothing, float gscale, float* grad, double* row_loss, int* row_stat,
                        void* stream);
/* out4 = {loss_ctc, loss_att, acc, loss}; denom <= 0 selects the length-normalised
 * attention loss (denominator = non-ignored targets, counted on device) and then also
 * writes out4[4] = 1 / that count (out4 must hold 5 floats). */
int esp_reduce_losses(const double* nll, int B, int zero_inf, const double* row_loss,
                      const int* row_stat, int R, float denom, float ctc_w, float* out4,
                      void* stream);
int esp_argmax(const float* x, long long* out, long rows, int V, void* stream);
int esp_ctc_forced_align(const float* lpz, int T, int V, const long long* y, int U, int blank,
                         int* path, long long* out, void* stream);
/* ABI 31: forced_align over a batch (replaces a loop of espnet/nets/pytorch_backend/ctc.py:185-249
 * CTC.forced_align calls, one per utterance): lpz (B, T, V) fp32 log-probs, utterance b uses its first
 * tlen[b] frames and the first ulen[b] labels of row b of y (B, Umax) int64 (tlen / ulen: device int32);
 * out (B, T) int64 labels, -1 past tlen[b] (and for an utterance with no frames or labels);
 * path: B * T * (2 Umax + 1) int32 workspace.  Each row equals esp_ctc_forced_align on that utterance. */
int esp_ctc_forced_align_batch(const float* lpz, int B, int T, int V, const int* tlen, const long long* y,
                               int Umax, const int* ulen, int blank, int* path, long long* out, void* stream);

/* ---- beam-search CTC prefix scoring (espnet/nets/ctc_prefix_score.py:279-359 CTCPrefixScore,
 *      espnet/nets/scorers/ctc.py CTCPrefixScorer; inference)
 * lp: one utterance's (T, V) CTC log-softmax.  States are (T, 2) fp32 rows (log r^n, log r^b).
 * init: r0 = initial state of the <sos> prefix.  score: for NH hypotheses (states r_prev
 * (NH, T, 2), last label last[NH], common output length out_len = len(prefix) - 1) and C
 * candidate labels each (cands (NH, C)), writes r_new (NH, C, T, 2) and log_psi (NH, C);
 * log_psi = log r^n+r^b at T-1 for c == eos, -1e10 for c == blank. */
int esp_ctc_prefix_init(const float* lp, int T, int V, int blank, float* r0, void* stream);
int esp_ctc_prefix_score(const float* lp, int T, int V, const float* r_prev, const long long* last,
                         int out_len, const long long* cands, int NH, int C, int blank, int eos,
                         float* r_new, float* log_psi, void* stream);
/* ABI 35: esp_ctc_prefix_score for the hypotheses of several utterances in one launch (the lockstep search of
 * BatchBeamSearch.forward_batch; same recursion, espnet/nets/ctc_prefix_score.py CTCPrefixScoreTH's batch form):
 * lp (U, Tmax, V), tlen (U) device int32 frames per utterance, utt (NH) device int32 utterance of each
 * hypothesis; states (NH, Tmax, 2), r_new (NH, C, Tmax, 2).  Frames at or beyond tlen[utt] do not contribute
 * (the <eos> score is taken at frame tlen - 1; state rows past it are logzero).  A hypothesis whose utterance,
 * length or candidate label is out of range reads nothing and scores logzero. */
int esp_ctc_prefix_score_batch(const float* lp, int U, int Tmax, int V, const int* tlen, const int* utt,
                               const float* r_prev, const long long* last, int out_len, const long long* cands,
                               int NH, int C, int blank, int eos, float* r_new, float* log_psi, void* stream);

/* ABI 40: growing CTC prefix states to a longer encoder window (the block-synchronous beam search;
 * espnet/nets/ctc_prefix_score.py:245-270 CTCPrefixScoreTH.extend_state).  r (NH, Tmax, 2) in place: for the frames
 * t in [max(t_old, 1), t_new), r[h, t, 0] = -1e10 and r[h, t, 1] = r[h, t-1, 1] + lp[utt[h], t, blank] (only the
 * blank path of an already scored prefix goes on); fp32 adds in frame order, one thread per hypothesis.  Rows
 * outside that range are not written; a hypothesis whose utterance is out of range is left alone.
 * 0 <= t_old <= t_new <= Tmax (else status -1); t_old == t_new writes nothing. */
int esp_ctc_prefix_extend(const float* lp, int U, int Tmax, int V, const int* utt, float* r, int NH, int t_old,
                          int t_new, int blank, void* stream);

/* ABI 40: row gather of a decoder K/V cache into a second buffer (csrc/decode_attn.hip; DecoderCache.reorder_keep):
 *   dst[l, i, p, :] = src[l, index[i], p, :]  for l < NL, i < n, p < len
 * src (NL, src_R, src_C, W) and dst (NL, dst_R, dst_C, W) fp32, distinct and 16-byte aligned, W a multiple of 4;
 * index: n device int64, may repeat; an entry outside [0, src_n) moves nothing.  src is left as it is, which is what
 * lets a search take one step back.  n <= dst_R, src_n <= src_R, len <= src_C and dst_C (else status -1). */
int esp_cache_gather(const float* src, float* dst, const long long* index, int NL, int n, int len, int W, int src_n,
                     int src_R, int src_C, int dst_R, int dst_C, void* stream);

/* ---- ABI 35: single-query attention of the cached decoder step (csrc/decode_attn.hip; replaces
 * MultiHeadedAttention on a one-row query in TransformerDecoder.forward_one_step,
 * espnet2/asr/decoder/transformer_decoder.py:147-190):
 *   out[n, h] = softmax(q[n, h] . K[src[n], :klen[n], h] / sqrt(dk)) . V[src[n], :klen[n], h]
 * for N rows and H heads, fp32, online softmax over 64-key chunks.  q row n at q + n*ldq + qoff + h*dk; key j
 * of source sequence s at k + s*sk + j*ldk + koff + h*dk (v alike, so K and V may share one fused buffer); out
 * row n at out + n*ldo + ooff + h*dk.  idx_host / idx_dev: the same 2N int32 on the host and on the device,
 * src[0..N) then klen[0..N).  The host copy is checked (0 <= src < nsrc, 1 <= klen <= Tk: status -1), the
 * kernel reads the device copy; keys at or beyond klen[n] are never read.  dk 16, 32 or 64 (else -1);
 * q / K / V pointers 16-B aligned, their strides and offsets multiples of 4 floats. */
int esp_decode_attn(const float* q, long ldq, long qoff, const float* k, long ldk, long sk, long koff,
                    const float* v, long ldv, long sv, long voff, float* out, long ldo, long ooff,
                    const int* idx_host, const int* idx_dev, int N, int H, int dk, int nsrc, int Tk, void* stream);

/* ---- ABI 36: the Transformer LM step (shallow fusion; espnet2/lm/transformer_lm.py batch_score over
 * espnet/nets/pytorch_backend/transformer/encoder.py forward_one_step).
 *
 * esp_decode_attn_masked (csrc/decode_attn.hip): esp_decode_attn with a per-row key-validity byte mask, row n at
 * mask + n*ldm (ldm >= the longest klen): key j of row n takes part when j < klen[n] and mask[n*ldm + j] != 0 (the LM hides the
 * keys whose token id is 0).  Masked keys are never read.  Every row needs at least one valid key.  With an
 * all-ones mask the result equals esp_decode_attn's bit for bit.
 *
 * esp_step_linear (csrc/lm_step.hip): out[n, :] = act(LN?(x[n, :]) . W^T + b) (+ R[n, :]) for N decode rows, W
 * (M, K) row-major with pitch ldw, fp32 FMA; the weight is streamed once per tile of 8 rows.  ln_gamma / ln_beta
 * (both or neither): LayerNorm over K with ln_eps before the product.  bias, R NULL: absent.  relu != 0: ReLU before
 * the residual.  Columns [0, c0) are stored to out + n*ldo; columns [c0, M) to
 * out2 + n*row_stride2 + pos*(M - c0) + (m - c0), the position-`pos` slot of row n of a (rows2, capacity2, M - c0)
 * buffer with row pitch row_stride2 (a DecoderCache layer: K | V written in place).  c0 = M: no split (out2 may be
 * NULL).  The split store is checked on the host (0 <= pos < capacity2, N <= rows2, row_stride2 >= capacity2*(M-c0):
 * status -1).  K a multiple of 4, at most 2048; x / W rows 16-byte aligned.  R may be `out`.
 *
 * esp_step_ln_act (csrc/lm_step.hip): y[r, :] = relu(LN(x[r, :])) * xscale + pe[pos0 + r % L, :] for `rows`
 * contiguous rows of D floats (pe NULL: y = relu(LN(x)), the identity positional step); pe has pe_rows rows. */
int esp_decode_attn_masked(const float* q, long ldq, long qoff, const float* k, long ldk, long sk, long koff,
                           const float* v, long ldv, long sv, long voff, float* out, long ldo, long ooff,
                           const int* idx_host, const int* idx_dev, const unsigned char* mask, long ldm, int N, int H,
                           int dk, int nsrc, int Tk, void* stream);
int esp_step_linear(const float* x, long ldx, const float* W, long ldw, const float* bias, const float* ln_gamma,
                    const float* ln_beta, float ln_eps, int relu, const float* R, long ldr, float* out, long ldo, int c0,
                    float* out2, long row_stride2, int pos, int capacity2, int rows2, int N, int K, int M, void* stream);
int esp_step_ln_act(const float* x, const float* gamma, const float* beta, float eps, float xscale, const float* pe,
                    int L, int pos0, int pe_rows, float* y, int rows, int D, void* stream);

/* ---- ABI 38: the contextual block Transformer encoder (csrc/cbt.hip;
 * espnet2/asr/encoder/contextual_block_transformer_encoder.py forward_train).
 *
 * esp_block_attn_fwd / _bwd: self-attention over Z independent sequences of S slots, one workgroup per (sequence,
 * head), exact fp32 FMA, nothing but ctx and the row log-sum-exp written.  qkv: (Z*S, 3*H*dk) rows q | k | v (the
 * fused projection's output); ctx: (Z*S, H*dk); lse: Z*H*S floats.  Mask: key j takes part iff j <= S - 2; query
 * row 0 is dead (ctx row 0 = 0, no gradient through it as a query; as a key and value it is live).  Dropout on the
 * probabilities with the counter hash at index ((z*H + h)*64 + i)*64 + j.  The backward recomputes the
 * probabilities from qkv and lse, regenerates the mask, and writes dq | dk | dv into dqkv (Z*S, 3*H*dk) (every
 * element written).  3 <= S <= 64, dk 16, 32 or 64, 0 <= drop_p < 1 (else status -1); buffers 16-byte aligned.
 *
 * The block layout: T frames, block_size bs, hop, look_ahead la, nblk = ceil((T - bs + hop) / hop) blocks of
 * S = bs + 2 slots; T > bs >= 1, hop >= 1, la >= 0, bs - hop - la >= 0, nblk as stated (else status -1); bs itself is
 * not capped here (only esp_block_attn_* is limited to 64 slots).
 * esp_cbt_chunk_fwd: x (B, T, D) -> xs (B, nblk, S, D): slot s in 1..bs of block k holds frame t = k*hop + s - 1 as
 *   drop(x*xscale + pe[t]) (0 when t >= T), the mask keyed on (b, t, c) with seed_x so that a frame carries one mask
 *   in every block; slot bs + 1 holds the block's context vector, the mean of x over frames [k*hop, min(k*hop + bs, T)),
 *   taken through drop(mean*xscale + pe[k]) (mask keyed on (b, k, c) with seed_c) when ctx_pos_enc, and slot 0 the
 *   context vector of block max(k - 1, 0).  pe: (pe_rows >= max(T, nblk), D).
 * esp_cbt_chunk_bwd: dxs -> dx (B, T, D), a gather: every dx element sums the blocks that hold its frame and the
 *   means whose window holds it.
 * esp_cbt_ctx_shift_fwd (in place): xs[b, k, 0] = xs[b, max(k - 1, 0), S - 1].  _bwd (in place) is its adjoint:
 *   dxs[b, k, S - 1] += dxs[b, k + 1, 0] (+ dxs[b, 0, 0] for k = 0), then dxs[b, :, 0] = 0.
 * esp_cbt_unchunk_fwd: y[b, t] = xs[b, k, t - k*hop + 1], k = 0 for t < bs - la, else
 *   min((t - (bs - la)) / hop + 1, nblk - 1).  _bwd: dxs = the one-to-one scatter of dy, 0 elsewhere (every element
 *   written). */
int esp_block_attn_fwd(const float* qkv, float* ctx, float* lse, long Z, int S, int H, int dk, float drop_p,
                       unsigned long long seed, void* stream);
int esp_block_attn_bwd(const float* qkv, const float* dctx, const float* lse, float* dqkv, long Z, int S, int H, int dk,
                       float drop_p, unsigned long long seed, void* stream);
int esp_cbt_chunk_fwd(const float* x, const float* pe, int pe_rows, float* xs, int B, int T, int D, int bs, int hop,
                      int la, int nblk, float xscale, int ctx_pos_enc, float drop_p, unsigned long long seed_x,
                      unsigned long long seed_c, void* stream);
int esp_cbt_chunk_bwd(const float* dxs, float* dx, int B, int T, int D, int bs, int hop, int la, int nblk, float xscale,
                      int ctx_pos_enc, float drop_p, unsigned long long seed_x, unsigned long long seed_c, void* stream);
int esp_cbt_ctx_shift_fwd(float* xs, int B, int nblk, int S, int D, void* stream);
int esp_cbt_ctx_shift_bwd(float* dxs, int B, int nblk, int S, int D, void* stream);
int esp_cbt_unchunk_fwd(const float* xs, float* y, int B, int T, int D, int bs, int hop, int la, int nblk, void* stream);
int esp_cbt_unchunk_bwd(const float* dy, float* dxs, int B, int T, int D, int bs, int hop, int la, int nblk,
                        void* stream);

/* ---- ABI 41: Mask-CTC mask-predict decoding (csrc/maskctc.hip; espnet2/asr/maskctc_model.py
 * MaskCTCInference.forward).  One workgroup per utterance; selection only (max, argmax, rank).
 *
 * esp_maskctc_init (:288-317): lp (T, V) fp32, the CTC log-softmax of one utterance.  Per frame the maximum and its
 * first index; runs of equal ids are collapsed, blank runs dropped, and each remaining run (token) takes the maximum
 * log-probability of its frames: tok_logp[i], bit-equal to that fp32 maximum, tok_prob[i] = expf(tok_logp[i]).  Token
 * i is masked when (double)tok_prob[i] < threshold (the reference compares a Python float holding the fp32 value):
 * y_in[i] = mask_token, else the token id.  counts = {L, mask_num}: tokens and masked tokens.  y_in (int64),
 * tok_logp, tok_prob: T entries each, the first L written.  fid (int32) / flp (fp32): T entries of scratch (the
 * per-frame argmax and maximum).  exp is monotone, so the per-frame argmax of lp is the reference's argmax of
 * exp(lp) unless two distinct log-probabilities round to one probability.
 *
 * esp_maskctc_fill (:327-331, :336-337): logits (L, V1) fp32 raw decoder outputs, V1 = vocabulary + <mask>; y_in
 * (L) int64 in place.  Every position holding mask_token takes the maximum and first argmax of its row over all V1
 * classes (the mask token included, as the reference).  k > 0: the k masked positions with the largest maxima are
 * set to their argmax (rank by counting, the lower index first on equal maxima); k == 0: every masked position is.
 * 1 <= L <= 2048 (else status -1). */
int esp_maskctc_init(const float* lp, int T, int V, int blank, long long mask_token, double threshold, int* fid,
                     float* flp, long long* y_in, float* tok_logp, float* tok_prob, int* counts, void* stream);
int esp_maskctc_fill(const float* logits, int L, int V1, long long* y_in, long long mask_token, int k, void* stream);

/* The same two steps for U ragged utterances, one workgroup per utterance (grid = U), on the device bodies of the
 * entry points above: a U = 1 batch writes what they write, bit for bit.  No atomics, no workgroup waits for another.
 *
 * esp_maskctc_init_batch: lp (U, Tmax, V) fp32; tlens (U) device int32 (clamped to [0, Tmax]).  Utterance u reads
 * frames [0, tlens[u]) only.  y_in / tok_logp / tok_prob / fid / flp: (U, Tmax); row u's first L_u entries are
 * esp_maskctc_init's for that utterance alone, y_in[u, i >= L_u] = 0.  counts (U, 4) int32 = {L, mask_num, num_iter,
 * k}, the reference's pass plan (:319-323): num_iter = n_iterations if mask_num >= n_iterations > 0 else mask_num;
 * k = mask_num / num_iter (0 when num_iter == 0).
 *
 * esp_maskctc_fill_batch: pass t on logits (Ua, Lmax, V1) fp32; workgroup a serves utterance u = rows[a] (Ua device
 * int32, distinct, in [0, U); others are skipped): row u of y_in (U, ld) int64 in place, positions [0, L_u).
 * t >= num_iter_u: untouched (by the plan, not by "no masks left": a position whose argmax was <mask> in the last
 * pass stays); t < num_iter_u - 1: esp_maskctc_fill with k_u; t == num_iter_u - 1: with k = 0.
 * 1 <= Lmax <= 2048, ld >= Lmax (else status -1). */
int esp_maskctc_init_batch(const float* lp, const int* tlens, int U, int Tmax, int V, int blank, long long mask_token,
                           double threshold, int n_iterations, int* fid, float* flp, long long* y_in, float* tok_logp,
                           float* tok_prob, int* counts, void* stream);
int esp_maskctc_fill_batch(const float* logits, int Ua, int Lmax, int V1, long long* y_in, int ld, const int* counts,
                           const int* rows, int U, long long mask_token, int t, void* stream);

/* ---- ABI 42: Transformer LM training (espnet2/lm/transformer_lm.py forward, espnet2/lm/espnet_model.py).
 *
 * esp_causal_attn_fwd / _bwd (csrc/causal_attn.hip): causal self-attention of B sequences of L tokens, one workgroup
 * per (sequence, head), exact fp32 FMA, no dropout.  qkv: (B*L, 3*H*dk) rows q | k | v (the fused projection's
 * output); ctx / dctx: (B*L, H*dk); lse: B*H*L floats, row (b*H + h)*L + i; klen: B device int32 (clamped to [0, L]).
 * Key j is visible to query i iff j <= i and j < klen[b]; scale 1 / sqrt(dk).  The forward writes ctx and the row
 * log-sum-exp only; the backward recomputes the probabilities from qkv and lse and writes every element of dqkv
 * (dq | dk | dv; no pre-zeroing, no atomics, bit-reproducible).  Query rows i >= klen[b]: ctx = 0, lse = 0, dq = 0;
 * key rows j >= klen[b]: dk = dv = 0.  Served: dk in {16, 32, 64, 128}, 1 <= L <= 64 for every dk (dk = 128, L = 64:
 * 132 KiB of LDS in the backward); anything else: status -1, nothing launched.  qkv / ctx / dctx / dqkv 16-byte
 * aligned.
 *
 * esp_lm_front_fwd / _bwd (csrc/lm_step.hip): the LM input layer's tail in training form (espnet1 encoder.py
 * input_layer "linear": LayerNorm -> Dropout(p1) -> ReLU -> positional step), rows of D floats, row r at position
 * r % L:  y = drop2(relu(drop1(LN(x))) * xscale + pe[r % L]);  pe NULL (the empty positional step): y =
 * relu(drop1(LN(x))), no scale, no second dropout.  Dropout masks by element index r*D + c under seed1 / seed2.
 * The forward saves mean / rstd (rows floats each); at p1 = 0 its values equal esp_step_ln_act's bit for bit.
 * The backward takes dy, regenerates both masks, recomputes the ReLU decision from x and the saved statistics,
 * writes the gradient of LN(x) to dz (rows*D floats of scratch, distinct from dy and dx) and runs esp_layernorm_bwd
 * on it: dx (overwritten) the gradient of x, dgamma / dbeta accumulated (+=).  D % 4 == 0; work:
 * esp_layernorm_bwd_workspace_bytes(rows, D). */
int esp_causal_attn_fwd(const float* qkv, const int* klen, float* ctx, float* lse, int B, int L, int H, int dk,
                        void* stream);
int esp_causal_attn_bwd(const float* qkv, const int* klen, const float* dctx, const float* lse, float* dqkv, int B,
                        int L, int H, int dk, void* stream);
int esp_lm_front_fwd(const float* x, const float* gamma, const float* beta, float eps, float xscale, const float* pe,
                     int L, int pe_rows, float p1, unsigned long long seed1, float p2, unsigned long long seed2,
                     float* y, float* mean, float* rstd, int rows, int D, void* stream);
int esp_lm_front_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                     const float* rstd, float xscale, int has_pe, float p1, unsigned long long seed1, float p2,
                     unsigned long long seed2, float* dz, float* dx, float* dgamma, float* dbeta, int rows, int D,
                     float* work, long work_bytes, void* stream);

/* esp_conv1_dgrad (csrc/conv.hip): the feature gradient of the subsampling's first convolution (3 x 3, stride 2),
 * dx (B, T, F) = the adjoint of conv1 applied to dz1 (B, T1, F1, D) (ReLU mask already applied), W (D, 9).  Training
 * does not call it (the features are data); an encoder's run_backward forms it on request. */
int esp_conv1_dgrad(const float* dz1, const float* W, float* dx, int B, int T, int F, int D, void* stream);

/* ---- RNN-Transducer head (additive: no signature above changed).  espnet2/asr/espnet_model.py:542-588,
 * espnet2/asr_transducer/joint_network.py, espnet2/asr/decoder/transducer_decoder.py.  Lengths are device int32
 * arrays (hlens[b] = T_b frames, tlens[b] = U_b labels, clamped to the padded extents T and U1 - 1); blank is
 * token 0; U1 = Umax + 1 <= 1024 and B*T*U1 < 2^31, else status -1.
 *
 * esp_rnnt_joint_fwd (csrc/rnnt.hip): z (B, T, U1, J) = act(pe[b,t,:] + pd[b,u,:]), pe (B*T, J), pd (B*U1, J);
 * act 0 tanh, 1 relu; every cell of the padded extent is written.
 * esp_rnnt_joint_bwd: dz (B, T, U1, J) and the forward's z -> dpe[b,t,:] = sum_u dz act'(z), dpd[b,u,:] = sum_t
 * dz act'(z), every element written.  Cells with t >= T_b or u > U_b are not read and add exactly zero.  Fixed
 * summation order, no atomics (per-tile partials in `work`, then a reduce pass): bit-reproducible.
 *
 * The loss shares one fp64 workspace of esp_rnnt_loss_workspace_bytes(B, T, U1) = 5 B T U1 doubles: lse | lp_blank
 * | lp_y | alpha | beta, each (B, T, U1).
 * esp_rnnt_logprobs: logits (B*T*U1, V) fp32, any V >= 1; ys (B, U1 - 1) int64.  Per valid cell the max-shifted
 * log-sum-exp over V, the blank log-probability and (u < U_b) that of label ys[b,u]; padded cells: unread, zeros
 * in all five arrays.
 * esp_rnnt_alpha_beta: the lattice recursions, one workgroup per (utterance, direction), anti-diagonal sweep, fp64:
 * alpha[0,0] = 0, alpha[t,u] = lse(alpha[t-1,u] + lp_blank[t-1,u], alpha[t,u-1] + lp_y[t,u-1]); beta[T_b-1,U_b] =
 * lp_blank[T_b-1,U_b], beta[t,u] = lse(beta[t+1,u] + lp_blank[t,u], beta[t,u+1] + lp_y[t,u]); nll[b] =
 * -(alpha[T_b-1,U_b] + lp_blank[T_b-1,U_b]) (fp64; +inf when T_b <= 0).  Any T_b >= 1, U_b >= 0.
 * esp_rnnt_grad: overwrites the logits with the gradient of gscale * (gdev ? *gdev : 1) * sum_b nll_b w.r.t. them
 * (gdev: an optional device float, e.g. the upstream gradient of the loss); padded cells and utterances with a
 * non-finite nll: exactly 0. */
int esp_rnnt_joint_fwd(const float* pe, const float* pd, float* z, int B, int T, int U1, int J, int act, void* stream);
int esp_rnnt_joint_bwd(const float* dz, const float* z, const int* hlens, const int* tlens, float* dpe, float* dpd,
                       int B, int T, int U1, int J, int act, float* work, long work_bytes, void* stream);
int esp_rnnt_logprobs(const float* logits, const long long* ys, const int* hlens, const int* tlens, int B, int T,
                      int U1, int V, double* work, long work_bytes, void* stream);
int esp_rnnt_alpha_beta(const int* hlens, const int* tlens, int B, int T, int U1, double* work, long work_bytes,
                        double* nll, void* stream);
int esp_rnnt_grad(float* logits, const long long* ys, const int* hlens, const int* tlens, int B, int T, int U1, int V,
                  float gscale, const float* gdev, const double* nll, const double* work, long work_bytes,
                  void* stream);

/* esp_lstm_cell_fwd / _bwd (csrc/lstm.hip): one time step of a torch.nn.LSTM layer (gates i, f, g, o) for B rows of
 * H units, any H >= 1; every matrix is addressed by a pointer and a row pitch in floats, so a step reads and writes
 * slices of (B, U1, .) sequence buffers in place.  xproj: x W_ih^T + b_ih + b_hh of this step (4H per row).  The
 * forward adds hprev W_hh^T (W_hh (4H, H); exact fp32 FMA, fixed order; hprev / cprev NULL: zero state), writes the
 * gate activations to acts (4H per row; NULL: not kept), c to cout and h to hout and, when given, hout2.  The backward
 * takes dh (the gradient of h_u from above), dgnext (the pre-activation gate gradients of step u + 1, NULL at the last
 * step: the recurrent part dgnext W_hh is added inside), dc_in (B, H; the cell gradient carried from step u + 1, NULL:
 * zero) and writes dgates (4H per row; the gradient of xproj and of the recurrent product) and dc_out (B, H; may be
 * dc_in).  One launch per step. */
int esp_lstm_cell_fwd(const float* xproj, long ldx, const float* hprev, long ldh, const float* cprev, long ldc,
                      const float* Whh, float* acts, long lda, float* hout, long ldho, float* hout2, long ldho2,
                      float* cout, long ldco, int B, int H, void* stream);
int esp_lstm_cell_bwd(const float* dh, long lddh, const float* dgnext, long ldgn, const float* Whh, const float* acts,
                      long lda, const float* c, long ldc, const float* cprev, long ldcp, const float* dc_in,
                      float* dc_out, float* dgates, long ldg, int B, int H, void* stream);

/* ---- workspace sizes.  Every launcher that takes a scratch `work` buffer also takes its size
 * in bytes and fails (status -1, esp_last_error) when it is smaller than the size below, which is
 * computed by the same code that picks the launcher's chunking: callers size their buffers from
 * these queries, never from a restated formula.  Pure host arithmetic (no device call). */
long esp_grad_norm_workspace_bytes(long n);
long esp_layernorm_bwd_workspace_bytes(int M, int D);
long esp_colsum_workspace_bytes(int M, int N);
long esp_dwconv1d_wgrad_workspace_bytes(int Bn, int T, int D, int K);
long esp_ebf_merge_bwd_workspace_bytes(int B, int T, int C, int k);
long esp_bn_swish_fwd_workspace_bytes(int M, int D);
long esp_bn_swish_bwd_workspace_bytes(int M, int D);
long esp_conv1_wgrad_workspace_bytes(int B, int T, int F, int D);
long esp_conv2_dgrad_workspace_bytes(int D);
long esp_ctc_loss_workspace_bytes(int B, int T, int Umax);
long esp_rnnt_joint_bwd_workspace_bytes(int B, int T, int U1, int J);
long esp_rnnt_loss_workspace_bytes(int B, int T, int U1);
/* esp_relpos_dp adapts its grouping to the buffer it gets; this is its preferred size */
long esp_relpos_dp_workspace_bytes(int nb, int H, int T);

#ifdef __cplusplus
}
#endif
#endif
