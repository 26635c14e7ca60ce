/* libhoisdf_hip - C ABI of the MI355X (gfx950) HOISDF hot path.
 *
 * The reference (amathislab/HOISDF) has no FFI layer: its boundary for this path is the
 * Python surface Model.forward / sdf_forward / sdf_infer / get_input_transformer /
 * SDFDecoder.forward / Transformer.forward.  This header is the
 * C-ABI a binding for that surface calls into; every entry cites the reference lines it
 * replaces.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - all tensors are caller-allocated DEVICE buffers of float32 unless stated otherwise;
 *     the library never allocates, frees or retains caller memory;
 *   - every entry takes a HIP stream (hipStream_t passed as void*), is asynchronous, does
 *     no hidden synchronisation and keeps no mutable global state;
 *   - return value: 0 = ok, negative = hoisdf_status; the message of the last failure on
 *     the calling thread is available from hoisdf_last_error();
 *   - "rows" are point/token rows; `ld*` are leading dimensions in floats;
 *   - dropout: p in [0,1); the keep mask is a pure function of (seed, element index), the
 *     backward entry regenerates it from the same (p, seed).
 */
#ifndef HOISDF_H_
#define HOISDF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HOISDF_VERSION_MAJOR 0
#define HOISDF_VERSION_MINOR 1

typedef enum hoisdf_status {
  HOISDF_OK = 0,
  HOISDF_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, unsupported dim) */
  HOISDF_ERR_LAUNCH = -2,    /* HIP launch / runtime error */
  HOISDF_ERR_TOO_FEW = -3,   /* sdf_infer: fewer bbox survivors than requested points */
  HOISDF_ERR_WORKSPACE = -4  /* workspace too small */
} hoisdf_status;

#define HOISDF_MAX_LEVELS 8

/* Feature pyramid in NHWC (channels-last) layout: level l is [B][H[l]][W[l]][C[l]].
 * Concatenation order = level order (reference: cfg.mutliscale_layers, main/config.py:99). */
typedef struct hoisdf_pyramid {
  int n_levels;
  int B;
  const float* data[HOISDF_MAX_LEVELS];
  int C[HOISDF_MAX_LEVELS];
  int H[HOISDF_MAX_LEVELS];
  int W[HOISDF_MAX_LEVELS];
} hoisdf_pyramid;

typedef struct hoisdf_pyramid_grad {
  int n_levels;
  int B;
  float* data[HOISDF_MAX_LEVELS];
  int C[HOISDF_MAX_LEVELS];
  int H[HOISDF_MAX_LEVELS];
  int W[HOISDF_MAX_LEVELS];
} hoisdf_pyramid_grad;

const char* hoisdf_version(void);
const char* hoisdf_last_error(void);
/* Deterministic mode (also: environment HOISDF_DETERMINISTIC=1, read at first use).  Every entry that otherwise
 * accumulates with float atomics switches to an order-fixed form: two identical call sequences give bit-identical
 * results.  Contract: one stream at a time (the ordered block reductions share a library-owned scratch); grad-weight is
 * order-fixed only when the caller passes the workspace (hoisdf_linear_bwd_weight_workspace). */
void hoisdf_set_deterministic(int on);
/* the contractions inside composite entries as fp32 emulated on the bf16 MFMA pipe (hoisdf_linear_fwd_emu); default ON
 * (environment HOISDF_GEMM=f32 or hoisdf_set_gemm_emu(0): the exact-f32 MFMA kernel) */
void hoisdf_set_gemm_emu(int on);
int hoisdf_get_gemm_emu(void);
int hoisdf_get_deterministic(void);

/* ---- K1: pinhole projection + 5-level bilinear gather --------------------------------
 * reference: main/model.py:148-175 (get_input_transformer), :190-214 (sdf_forward),
 * :286-328 (sdf_infer); F.grid_sample(bilinear, border, align_corners=True).
 * points [n_rows][3] in the scaled SDF frame; row r belongs to sample
 * sample_idx[r] (int32) or r / rows_per_sample when sample_idx is NULL.
 * cam = p/scale + center[b]; uv = (K[b] cam)_xy / (K[b] cam)_z; grid = (uv - n)/n with
 * n = ((img_w-1)/2, (img_h-1)/2).  feat [n_rows][ldf] receives the concatenated levels;
 * cam_out [n_rows][3] and uv_out [n_rows][2] are optional (may be NULL). */
int hoisdf_project_gather_fwd(const hoisdf_pyramid* pyr, const float* points,
                              const int32_t* sample_idx, long n_rows, int rows_per_sample,
                              const float* center, const float* cam_intr, float scale,
                              int img_h, int img_w, float* feat, int ldf, float* cam_out,
                              float* uv_out, void* stream);
/* Scatter-add of dfeat into the (pre-zeroed or accumulating) pyramid gradient. */
int hoisdf_project_gather_bwd(const hoisdf_pyramid_grad* dpyr, const float* points,
                              const int32_t* sample_idx, long n_rows, int rows_per_sample,
                              const float* center, const float* cam_intr, float scale,
                              int img_h, int img_w, const float* dfeat, int ldf, void* stream);

/* ---- K2/K7/K9/K11: fused linear layers (exact fp32 on the f32 MFMA pipe) --------------
 * reference: nn.Linear inside common/nets/layer.py:168-201 (MLP), common/nets/sdf_net.py
 * :87-113 (SDFDecoder hidden layers), nn.MultiheadAttention in/out projections and FFN
 * (common/nets/transformer.py:269-302).
 * y[M][N] = dropout(act(x[M][K] . W[N][K]^T + bias)), act: 0 none, 1 relu.
 * The dropout mask of element (m,n) is a hash of (seed, m, n).
 * relu_bits (optional, [M][ceil(N/32)] uint32): bit n%32 of word [m][n/32] is set iff
 * y[m][n] > 0, i.e. the element survived ReLU and dropout - all the backward needs. */
int hoisdf_linear_fwd(const float* x, int ldx, const float* W, int ldw, const float* bias,
                      float* y, int ldy, long M, int N, int K, int act, float drop_p,
                      uint64_t seed, uint32_t* relu_bits, void* stream);
/* Backward contractions.  If relu_bits (from the forward) is given, the ReLU + dropout backward
 * is fused into the load of dy: dy_eff = dy * bit / (1 - p); NULL means dy is used as is.
 * dx[M][K] = dy_eff[M][N] . W[N][K] */
int hoisdf_linear_bwd_input(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p,
                            const float* W, int ldw, float* dx, int lddx, long M, int N, int K,
                            int accumulate /* 1: dx += (the gradient another consumer of x already left there) */,
                            void* stream);
/* dW[N][K] = dy_eff[M][N]^T . x[M][K] ; db[N] = column sums of dy_eff (db may be NULL).
 * Split-K over M.  With a workspace of hoisdf_linear_bwd_weight_workspace(M,N,K) floats the
 * partial tiles are written there and summed by a second kernel: dW (dense, lddw == K) and db
 * are fully overwritten.  Without it (workspace == NULL) the kernel accumulates with float
 * atomics into dW / db, which the caller must have zero-filled (or hold gradients to add to). */
long hoisdf_linear_bwd_weight_workspace(long M, int N, int K);
int hoisdf_linear_bwd_weight(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p,
                             const float* x, int ldx, float* dW, int lddw, float* db, long M, int N,
                             int K, float* workspace, long workspace_floats, void* stream);
/* ---- fp32 linear layers emulated on the bf16 MFMA pipe ("bf16x3"; cfg.gemm_emu) ------------------------------------------
 * reference: the same call sites as hoisdf_linear_fwd / hoisdf_linear_bwd_input (common/nets/layer.py:168-201,
 * common/nets/transformer.py:286-302, main/model.py:56-90).  Same contracts and argument meaning, fp32-equivalent results:
 * every f32 operand is split EXACTLY into three bf16 pieces (8 + 8 + 8 significand bits, no scaling - bf16 has the f32
 * exponent range) and each product is accumulated in f32 from six bf16 MFMA products (the three dropped cross terms are
 * <= 2^-24 of the product); error against fp64 = that of the exact-f32 entries (tests/test_gpu_emu.py), not bit-identical
 * to them (another summation order).  The weight operand is handed over as a pre-split "slab image"
 * (hoisdf_linear_emu_image_bytes(rows, K) bytes, 16-byte aligned, caller-owned):
 *   hoisdf_linear_emu_prepare(W, ldw, N, K, 0, image)  -> image for hoisdf_linear_fwd_emu       (rows = N, contraction K)
 *   hoisdf_linear_emu_prepare(W, ldw, N, K, 1, image)  -> image for hoisdf_linear_bwd_input_emu (rows = K, contraction N)
 * to be rebuilt whenever W changes (once per optimizer step).  The activation operand must be 16-byte aligned with a leading
 * dimension and a contraction length that are multiples of 4 (hoisdf_linear_emu_supported); other shapes stay on the f32
 * entries. */
long hoisdf_linear_emu_image_bytes(int rows, int K);
int hoisdf_linear_emu_prepare(const float* W, int ldw, int N, int K, int transpose, void* image, void* stream);
/* All images of a model in ONE launch (after an optimizer step: ~170 weights x two orientations in the reference's hot path,
 * a few microseconds each when built one by one).  `d_items` is a DEVICE table of n items, first_block ascending from 0
 * (item i occupies hoisdf_linear_emu_prepare_blocks(N, K, transpose) blocks), total_blocks = the sum. */
typedef struct hoisdf_emu_prep_item {
  const float* W;          /* [N][ldw] */
  void* image;             /* hoisdf_linear_emu_image_bytes(transpose ? K : N, transpose ? N : K) bytes, 16-byte aligned */
  long first_block;
  int ldw, N, K, transpose;
} hoisdf_emu_prep_item;
long hoisdf_linear_emu_prepare_blocks(int N, int K, int transpose);
int hoisdf_linear_emu_prepare_batch(const hoisdf_emu_prep_item* d_items, int n, long total_blocks, void* stream);
int hoisdf_linear_emu_supported(const float* a, long lda, int contraction);
/* ---- the two arithmetic forms of the emulated entries (process-wide; environment HOISDF_EMU_FORM, read at first use) -----------
 * "b3"  bf16x3: the exact three-piece split described above, six products per product, any operand range.
 * "h2"  f16x2 (default since round 5): every operand is scaled by a power of two s that puts its largest magnitude in
 *       [2^13, 2^14) and split into TWO f16 pieces, x s = hi + lo + r with |r| <= max(2^-22 |x s|, 2^-25): 22 significant bits
 *       (on average 2^-24 relative, the rounding of an f32 operation) for every element within 2^-16 of the largest one sharing its
 *       scale, an ABSOLUTE error of 2^-38 of that largest one below (the low piece is an f16 subnormal there); each product is
 *       accumulated in f32 from THREE f16 MFMA products (lo hi + hi lo + hi hi; the dropped lo lo term is <= 2^-22 of the product) and
 *       the result is scaled back.  Half the matrix-pipe work of b3.  Error against fp64 on the model's operands: that of b3 and of
 *       the exact-f32 entries (tests/test_gpu_emu.py, test_gpu_bench_geometry.py).
 *       WHO SHARES A SCALE (round 6): a weight matrix has one scale (kept in its image).  The row operand of a forward / grad-input
 *       contraction has ONE SCALE PER ROW (token): a row's rounding depends on that row alone, so the samples of a batch do not
 *       influence each other's results (sample 0 of a batch is bit-identical whatever the other samples are) and a row far below
 *       the matrix maximum keeps its 22 bits.  The grad-weight contracts over the rows: each of its row slices takes the largest
 *       magnitude of its own rows.  The attention operands (Q, K, V, dO) have one scale per (sample, head).
 *       The scales need the magnitudes at launch time.  ROW MAGNITUDES of a matrix of M rows: hoisdf_mag_words(M) = M u32 words, word
 *       r = the IEEE bits of max |x[r][:]| (or of an upper bound), ZERO-FILLED before the producer(s) run: the *_mag entries below
 *       fold their output's into y_mag / dx_mag with an unsigned atomic max per row and column tile (not with accumulate = 1), so do
 *       the LayerNorm, gather, positional-encoding, SDF-head and attention entries of the composite calls.  Without words (x_mag =
 *       NULL, and in the plain entries) the library measures the operand itself: one more read of it (hoisdf_mag_measure does the
 *       same once for several consumers).  HEAD MAGNITUDES of an attention operand matrix (rows = B samples x L tokens, groups of 64
 *       columns = heads): hoisdf_head_mag_words(M, groups, L) words, word[group * B + sample] = the IEEE bits of the maximum magnitude
 *       of THAT sample's rows in the group, exactly, for any L; zero-filled, then left by hoisdf_linear_fwd_emu_heads /
 *       hoisdf_linear_bwd_input_emu_heads / the composite entries, or made by hoisdf_head_mag_measure.  (The GEMM epilogue folds them
 *       where each of its 128-row sub-tiles lies inside one sample - L and M multiples of 128; otherwise those entries read the stored
 *       matrix once more, as hoisdf_head_mag_measure does: one more launch on the same stream, the same words.)
 *       A word SMALLER than the true maximum (a stale array) cannot make Inf / NaN: the splitting kernels run with f16 saturation
 *       on (MODE.FP16_OVFL) - up to 4x too small is harmless (head room of the [2^13, 2^14) target), beyond that the row's largest
 *       elements clip at 65504 / scale.
 * hoisdf_linear_emu_pieces() = 2 (h2) or 3 (b3).  The image format follows the form: images are built and consumed in one process. */
int hoisdf_linear_emu_pieces(void);
long hoisdf_mag_words(long rows);
/* the row magnitudes of a matrix whose producer left none: every word is written (no clearing needed); one read of x */
int hoisdf_mag_measure(const float* x, long ldx, long M, int K, uint32_t* words, void* stream);
long hoisdf_head_mag_words(long M, int groups, int L);
/* the head magnitudes of x[M][>= groups * 64] (samples of L consecutive rows): clears `words`, then one read of x */
int hoisdf_head_mag_measure(const float* x, long ldx, long M, int groups, int L, uint32_t* words, void* stream);
/* hoisdf_linear_fwd_emu_mag that also leaves the head magnitudes of the stored y (N % 64 == 0; zero-filled `y_heads`, samples of L rows,
 * any L: each sample's own maximum; L or M not a multiple of 128: y 16-byte aligned, ldy % 4 == 0) - what an attention in-projection
 * leaves for hoisdf_attention_fwd_emu_mag; y_mag may be NULL */
int hoisdf_linear_fwd_emu_heads(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M, int N,
                                int K, const uint32_t* x_mag, uint32_t* y_mag, uint32_t* y_heads, int L, void* stream);
/* the same for a grad-input (no sign bitmap, no accumulation): what an out-projection's backward leaves for the dO operand of
 * hoisdf_attention_bwd_emu_mag (K % 64 == 0: the heads are the columns of dx) */
int hoisdf_linear_bwd_input_emu_heads(const float* dy, int lddy, const void* wt_image, float* dx, int lddx, long M, int N, int K,
                                      const uint32_t* dy_mag, uint32_t* dx_mag, uint32_t* dx_heads, int L, void* stream);
int hoisdf_linear_fwd_emu_mag(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M, int N,
                              int K, int act, float drop_p, uint64_t seed, uint32_t* relu_bits, const uint32_t* x_mag,
                              uint32_t* y_mag, void* stream);
int hoisdf_linear_bwd_input_emu_mag(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const void* wt_image,
                                    float* dx, int lddx, long M, int N, int K, int accumulate, const uint32_t* dy_mag,
                                    uint32_t* dx_mag, void* stream);
/* grad-weight in the f16x2 form (h2 processes, 256-wide tiles; otherwise identical to hoisdf_linear_bwd_weight_emu, whose
 * bf16x3 arithmetic needs no magnitudes and stays available in either process form): dy_mag / x_mag as above, NULL = measured. */
int hoisdf_linear_bwd_weight_emu_mag(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x, int ldx,
                                     float* dW, int lddw, float* db, long M, int N, int K, float* workspace, long workspace_floats,
                                     const uint32_t* dy_mag, const uint32_t* x_mag, void* stream);
int hoisdf_linear_fwd_emu(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M, int N,
                          int K, int act, float drop_p, uint64_t seed, uint32_t* relu_bits, void* stream);
int hoisdf_linear_bwd_input_emu(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const void* wt_image,
                                float* dx, int lddx, long M, int N, int K, int accumulate, void* stream);
/* The same three contractions for SMALL row counts (M <= hoisdf_linear_emu_small_max_rows() = 2047: the 17-query decoder stack,
 * common/nets/transformer.py:366-395, and the regression heads - ~100 calls of 544 x 256 x 256 per training step that the tiled
 * kernels cut into a handful of tiles): one wave per 32 x 32 output tile, operands read from the f32 matrices themselves (no
 * weight image, no workspace), same arithmetic (exact three-way bf16 split, six products, f32 accumulation), same epilogues and
 * sign-map convention as the entries above.  Operands 16-byte aligned, leading dims / N / K multiples of 4
 * (hoisdf_linear_emu_small_supported).  The grad-weight form OVERWRITES dW (any lddw >= K) and db, order-fixed (no atomics). */
int hoisdf_linear_emu_small_max_rows(void);
int hoisdf_linear_emu_small_supported(const float* a, long lda, const float* W, long ldw, long M, int N, int K);
int hoisdf_linear_fwd_emu_small(const float* x, int ldx, const float* W, int ldw, const float* bias, float* y, int ldy, long M,
                                int N, int K, int act, float drop_p, uint64_t seed, uint32_t* relu_bits, void* stream);
int hoisdf_linear_bwd_input_emu_small(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* W, int ldw,
                                      float* dx, int lddx, long M, int N, int K, int accumulate, void* stream);
int hoisdf_linear_bwd_weight_emu_small(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x, int ldx,
                                       float* dW, int lddw, float* db, long M, int N, int K, void* stream);
/* dW[N][K] = dy_eff[M][N]^T . x[M][K], db[N] = column sums of dy_eff (db may be NULL), same emulation: both activation operands
 * are split into bf16 triples inside the kernel (a register transpose per 4-column x 8-row patch, no transposed copy through
 * HBM).  dW (dense: lddw == K) and db are fully OVERWRITTEN; the rows are split over the workgroups into partial tiles in
 * `workspace` (hoisdf_linear_bwd_weight_emu_workspace(M, N, K) floats, 16-byte aligned) and summed in slice order: no atomics,
 * run-to-run identical.  N, K, lddy, ldx multiples of 4, 16-byte aligned operands. */
long hoisdf_linear_bwd_weight_emu_workspace(long M, int N, int K);
int hoisdf_linear_bwd_weight_emu(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x, int ldx,
                                 float* dW, int lddw, float* db, long M, int N, int K, float* workspace, long workspace_floats,
                                 void* stream);
/* dpre = dy * (y > 0) * 1/(1-p): backward of relu followed by dropout, given the
 * post-dropout output y (an element is kept-and-positive iff y > 0).  In place allowed. */
int hoisdf_relu_dropout_bwd(const float* y, int ldy, const float* dy, int lddy, float* dpre,
                            int ldd, long M, int N, float drop_p, void* stream);

/* ---- K3/K4: SDF decoder pieces ---------------------------------------------------------
 * reference: common/utils/sdf_utils.py:96-141 (Embedder), main/model.py:218-228 (decoder
 * input [feat | posenc | xyz]), common/nets/sdf_net.py:57-62 (weight norm).
 * Writes columns [col0, col0+30) = posenc(points) and [col0+30, col0+33) = points of the
 * decoder-input rows x0 (ld = ldx0, trailing pad columns up to ldx0 zeroed), and the
 * stand-alone posenc rows pe [n_rows][30] (may be NULL). */
int hoisdf_posenc_fwd(const float* points, long n_rows, float* x0, int ldx0, int col0,
                      float* pe, void* stream);
/* W[r][:] = g[r] * v[r][:] / ||v[r][:]||, written with leading dimension ldw (>= in);
 * pad columns are zeroed.  norms[r] (optional) receives ||v[r]||. */
int hoisdf_weightnorm_fwd(const float* v, const float* g, float* W, int ldw, float* norms,
                          int out, int in, void* stream);
/* dv, dg from dW (same ldw): dg[r] = <dW[r], v[r]>/||v[r]||,
 * dv[r] = g[r]/||v[r]|| * (dW[r] - v[r] <dW[r], v[r]>/||v[r]||^2). */
int hoisdf_weightnorm_bwd(const float* v, const float* g, const float* dW, int ldw, float* dv,
                          float* dg, int out, int in, void* stream);
/* Final 512 -> 1 layer + tanh + clamp (common/nets/sdf_net.py:115-122, main/model.py:241).
 * sdf_raw = tanh(h . w + b) (unclamped, what sdf_infer sorts on); sdf = clamp(sdf_raw). */
int hoisdf_sdf_head_fwd(const float* h, int ldh, const float* w, const float* b, float* sdf_raw,
                        float* sdf, long n_rows, int K, float clamp, void* stream);
int hoisdf_sdf_head_bwd(const float* dsdf, const float* sdf_raw, const float* h, int ldh,
                        const float* w, float* dh, int lddh, float* dw, float* db, long n_rows,
                        int K, float clamp, void* stream);

/* ---- K1-K4 behind one call: the gradient-free SDF query ----------------------------------------------------
 * reference: Model.sdf_forward (main/model.py:181-244) and the body of Model.sdf_infer (:285-354) - project + gather,
 * linear_sdfin, positional encoding, SDFDecoder, tanh + clamp - for the call sites whose results are only ever used
 * detached (:483-484,:517-518,:540,:558) and for inference.  SURVEY.md section 8(b) `hoisdf_sdf_query_fwd`.
 * Weights: plain device pointers; the four decoder matrices are EFFECTIVE weights (weight-norm folded,
 * hoisdf_weightnorm_fwd), two of them laid out for the in-place skip-concatenation:
 *   dec_w1 [224][512]  rows 0..222 = layer 1, row 223 = 0 (and dec_b1[223] = 0): the extra output is the zero pad column;
 *   dec_w2 [512][516]  columns 0..222 = W2[:, 0:223] (h1), 223 = 0, 224..512 = W2[:, 223:512] (x0), 513..515 = 0.
 * feat_in  (optional) [n_rows][C]: rows already gathered for these camera points (skips K1; cam_out must be NULL);
 * feat_out (optional) [n_rows][C]: receives the gathered rows for other consumers of the same points.
 * drop_p / seed: dropout after the decoder's hidden ReLUs (the module's train() mode; 0 in eval), layer i draws
 * stream seed + i of the counter hash.
 * Outputs: sdf (clamped), sdf_raw (tanh, unclamped: what sdf_infer ranks on), pe [n_rows][30] (optional),
 * cam_out [n_rows][3] (optional).  workspace: hoisdf_sdf_query_workspace(n_rows, C, need_feat) bytes, need_feat = 1
 * when neither feat_in nor feat_out is given. */
typedef struct hoisdf_sdf_weights {
  int C;                                  /* pyramid channels (992 / 3968) */
  const float *sdfin_w0, *sdfin_b0;       /* [512][C], [512] */
  const float *sdfin_w1, *sdfin_b1;       /* [256][512], [256] */
  const float *dec_w0, *dec_b0;           /* [512][dec_ld0 >= 289], [512] */
  int dec_ld0;
  const float *dec_w1, *dec_b1;           /* [224][512], [224] */
  const float *dec_w2, *dec_b2;           /* [512][516], [512] */
  const float *dec_w3, *dec_b3;           /* [512][512], [512] */
  const float *dec_w4, *dec_b4;           /* [512], [1] */
  /* optional (NULL = built per call in the workspace): bf16x3 slab images (hoisdf_linear_emu_prepare) of the six matrices
   * sdfin_w0, sdfin_w1, dec_w0 .. dec_w3 in this order - emu_img for the forward GEMMs, emu_img_t (transpose = 1) for the
   * grad-input GEMMs of hoisdf_sdf_query_bwd.  The caller rebuilds them whenever it re-folds the weights (one
   * hoisdf_linear_emu_prepare_batch launch); a training step otherwise builds 48 images inside these entries. */
  const void* emu_img[6];
  const void* emu_img_t[6];
} hoisdf_sdf_weights;
long hoisdf_sdf_query_workspace(long n_rows, int C, int need_feat);
int hoisdf_sdf_query_fwd(const hoisdf_pyramid* pyr, const float* points, const int32_t* sample_idx, long n_rows,
                         int rows_per_sample, const float* center, const float* cam_intr, float scale, int img_h,
                         int img_w, const float* feat_in, float* feat_out, const hoisdf_sdf_weights* w, float clamp,
                         float drop_p, uint64_t seed, float* sdf, float* sdf_raw, float* pe, float* cam_out,
                         void* workspace, long workspace_bytes, void* stream);

/* ---- K5/K6: dense-grid candidate generation + selection (sdf_infer) -------------------
 * reference: main/model.py:257-302 (sheared lattice + strict bbox filter, on CPU there) and
 * :345-352 (sort by |sdf|, keep the first num_points).
 * Pass 1 (count) + pass 2 (fill) stream compaction of the bins_n^3 lattice per sample:
 *   counts [B] int32 survivors per sample;
 *   with offsets [B] (exclusive prefix of counts) the fill pass writes, for each survivor in
 *   ascending lattice order, points [n][3] (scaled frame), sample_idx [n] and lattice_idx [n].*/
int hoisdf_lattice_count(const float* center, const float* cam_intr, const float* bbox, float scale,
                         int bins_n, int B, int32_t* counts, void* stream);
int hoisdf_lattice_fill(const float* center, const float* cam_intr, const float* bbox, float scale,
                        int bins_n, int B, const int32_t* offsets, float* points,
                        int32_t* sample_idx, int32_t* lattice_idx, void* stream);
/* Per sample b, select the k rows with the smallest |sdf_raw| among rows
 * [offsets[b], offsets[b]+counts[b]) (ties: lower row first) and emit them in ascending
 * (|sdf|, row) order: sel [B][k] int32 global row indices.  Exact (radix select + rank).
 * Keys compare by the bit pattern of |x|: +0 and -0 tie, Inf sorts after every finite value and NaN after Inf.
 * The caller checks counts[b] >= k.  A sample with counts[b] < k is not an error here: its k entries of sel are all -1 and
 * the other samples are unaffected; hoisdf_gather_rows writes a row of zeros for an index of -1. */
int hoisdf_select_smallest_abs(const float* sdf_raw, const int32_t* offsets, const int32_t* counts,
                               int B, int k, int32_t* sel, void* stream);
/* out[r][0:width] = src[sel[r]][0:width]; sel[r] < 0: out[r][0:width] = 0 */
int hoisdf_gather_rows(const float* src, int lds, const int32_t* sel, long n_sel, int width,
                       float* out, int ldo, void* stream);
/* ---- the training-time SDF query, one call per direction (SURVEY.md section 8(b) `hoisdf_sdf_query_bwd`) ------------------
 * reference: Model.sdf_forward with gradients (main/model.py:181-244; the two SDF-loss queries of a training step).
 * hoisdf_sdf_query_train_fwd = the dataflow of hoisdf_sdf_query_fwd keeping, in `saved` (hoisdf_sdf_query_train_saved_bytes),
 *   what the backward needs: gathered rows, activations, the six ReLU / dropout sign bitmaps, the tanh output.
 * hoisdf_sdf_query_bwd: d_sdf [n_rows] (gradient of the CLAMPED sdf) -> weight gradients in the layouts of hoisdf_sdf_weights
 *   (d_dec_w0 [512][292]: the 289 real columns + the three zero pad columns of the decoder-input row; d_dec_w1 [224][512] and d_dec_b1 [224] with the pad row; d_dec_w2 [512][516] with the pad
 *   columns; all zero on entry), and the pyramid gradient scatter-ADDED into dpyr (NULL: skipped).  The weight-norm fold's own
 *   backward (hoisdf_weightnorm_bwd on the effective-weight gradients) is the caller's. */
typedef struct hoisdf_sdf_weight_grads {
  float *d_sdfin_w0, *d_sdfin_b0, *d_sdfin_w1, *d_sdfin_b1;
  float *d_dec_w0, *d_dec_b0, *d_dec_w1, *d_dec_b1, *d_dec_w2, *d_dec_b2, *d_dec_w3, *d_dec_b3, *d_dec_w4, *d_dec_b4;
} hoisdf_sdf_weight_grads;
long hoisdf_sdf_query_train_saved_bytes(long n_rows, int C);
long hoisdf_sdf_query_train_workspace_bytes(long n_rows, int C, int backward_pass);
int hoisdf_sdf_query_train_fwd(const hoisdf_pyramid* pyr, const float* points, const int32_t* sample_idx, long n_rows,
                               int rows_per_sample, const float* center, const float* cam_intr, float scale, int img_h, int img_w,
                               const hoisdf_sdf_weights* w, float clamp, float drop_p, uint64_t seed, float* sdf, float* pe,
                               float* cam_out, void* saved, long saved_bytes, void* workspace, long workspace_bytes, void* stream);
int hoisdf_sdf_query_bwd(const hoisdf_pyramid_grad* dpyr, const float* points, const int32_t* sample_idx, long n_rows,
                         int rows_per_sample, const float* center, const float* cam_intr, float scale, int img_h, int img_w,
                         const hoisdf_sdf_weights* w, float clamp, float drop_p, const void* saved, long saved_bytes,
                         const float* d_sdf, const hoisdf_sdf_weight_grads* grads, void* workspace, long workspace_bytes,
                         void* stream);

/* ---- sdf_infer in two calls (SURVEY.md section 8(b) `hoisdf_sdf_infer`) ----------------------------------------------
 * reference: Model.sdf_infer (main/model.py:246-355): dense sheared lattice inside the bbox -> SDF of every survivor ->
 * the num_points survivors of every sample with the smallest |sdf| (ascending) -> their points (scaled frame), clamped
 * SDF values and positional encodings.
 * hoisdf_sdf_infer_count_begin: queues the survivor count per sample into counts_device [B] and its copy into counts_host [B]
 *   (page-locked host memory that stays alive until the stream has executed the copy) and RETURNS WITHOUT WAITING.  The counts
 *   depend only on center / cam_intr / bbox (main/model.py:286-302), so a host can issue this ahead of the image encoder,
 *   record an event behind it and wait for that event when it reaches sdf_infer - no pipeline drain.
 * hoisdf_sdf_infer_count: the same followed by hipStreamSynchronize(stream) - the ONE blocking device -> host read of the
 *   path, for hosts that do not overlap it; *n_rows = the total.  The caller sizes the workspace with
 *   hoisdf_sdf_infer_workspace(n_rows, B, C) and calls
 * hoisdf_sdf_infer: exclusive scan of the counts (device) -> lattice fill -> hoisdf_sdf_query_fwd ->
 *   hoisdf_select_smallest_abs -> hoisdf_gather_rows.  It only enqueues work (no host <-> device copy, no synchronisation);
 *   counts_host is read on the host for validation and sizing.  A sample with fewer than num_points survivors is refused
 *   (the reference raises at main/model.py:348).
 *   points_out [B][num_points][3], sdf_out [B][num_points], pe_out [B][num_points][30] (optional). */
int hoisdf_sdf_infer_count_begin(const float* center, const float* cam_intr, const float* bbox, float scale, int bins_n,
                                 int B, int32_t* counts_device, int32_t* counts_host, void* stream);
int hoisdf_sdf_infer_count(const float* center, const float* cam_intr, const float* bbox, float scale, int bins_n, int B,
                           int32_t* counts_device, int32_t* counts_host, long* n_rows, void* stream);
long hoisdf_sdf_infer_workspace(long n_rows, int B, int C);
int hoisdf_sdf_infer(const hoisdf_pyramid* pyr, const float* center, const float* cam_intr, const float* bbox, float scale,
                     int bins_n, int B, const int32_t* counts_device, const int32_t* counts_host, int num_points, int img_h,
                     int img_w, const hoisdf_sdf_weights* w, float clamp, float drop_p, uint64_t seed, float* points_out,
                     float* sdf_out, float* pe_out, void* workspace, long workspace_bytes, void* stream);

/* ---- (f2) dataset-side SDF sample selection on the device ------------------------------------------------
 * reference: data/dexycb.py:514-546 (np.random.choice without replacement of num_samp_hand / num_samp_obj rows of
 * the frame's sdf_processed array, and - training - of the rows with |sdf| < points_filter_dist).
 * rows: HBM-resident store of sdf_processed rows [.. ld >= 6 floats: x y z sdf_hand sdf_obj label].  A segment s is
 * the row range [seg_row0[s], seg_row0[s] + seg_len[s]) of the store; seg_col[s] = 3 / 4 keeps only rows with
 * |row[col]| < dist eligible, -1 = all rows.  Writes keys[seg_off[s] + i] = uniform [0,1) (hash of seed, s, i) for
 * eligible rows, 1e30 otherwise, and eligible[s] = number of eligible rows.  Then
 * hoisdf_select_smallest_abs(keys, seg_off, seg_len, n_seg, k, sel) yields k uniformly drawn rows per segment
 * (indices into keys; the caller checks eligible[s] >= k) and hoisdf_gather_rows fetches them. */
int hoisdf_sdf_sample_keys(const float* rows, int ld, const int64_t* seg_row0, const int32_t* seg_len,
                           const int32_t* seg_off, const int32_t* seg_col, int n_seg, int max_len, float dist,
                           uint64_t seed, float* keys, int32_t* eligible, void* stream);

/* ---- K8: sigma gate + token assembly ----------------------------------------------------
 * reference: main/model.py:123-126 (sdf_activation), :520-562 (token concat).
 * For sample b and point p:  tok[b][row0+p][:] = [cam[b][p]-center[b] (3) | pe (30) |
 * feat[b][p][0:F] * sigmoid(sdf/beta)/beta],  beta = max(*beta_ptr, 2e-3), F = D - 33.
 * tok is batch-first [B][S][D]. */
int hoisdf_token_build_fwd(const float* cam, const float* center, const float* pe,
                           const float* feat, int ldfeat, const float* sdf, const float* beta_ptr,
                           float* tok, int B, int P, int S, int row0, int D, void* stream);
/* dfeat = dtok[33:] * sigma; *dbeta += sum dtok[33:] * feat * dsigma/dbeta (atomic). */
int hoisdf_token_build_bwd(const float* dtok, const float* feat, int ldfeat, const float* sdf,
                           const float* beta_ptr, float* dfeat, int lddfeat, float* dbeta, int B,
                           int P, int S, int row0, int D, void* stream);

/* The same with the beta gradient ORDER-FIXED: every block parks its partial sum in partials [hoisdf_token_build_bwd_partials()]
 * and a one-wave launch adds them to *dbeta in block order - run-to-run identical, and without the cross-block float atomics whose
 * order noise reached 1e-2 of this heavily cancelling scalar (hoisdf_amd/ops.py and hoisdf_tokens_bwd use this form). */
int hoisdf_token_build_bwd_partials(void);
int hoisdf_token_build_bwd_ordered(const float* dtok, const float* feat, int ldfeat, const float* sdf, const float* beta_ptr,
                                   float* dfeat, int lddfeat, float* dbeta, float* partials, int B, int P, int S, int row0,
                                   int D, void* stream);

/* ---- K9/K10: attention -------------------------------------------------------------------
 * reference: nn.MultiheadAttention as used by common/nets/transformer.py:286-302,366-395.
 * q rows [B][Lq][.. ldq], k/v rows [B][Lk][.. ldk/ldv], head h occupies columns
 * [h*64, h*64+64) of each.  Only the first kv_len keys are attended (memory_mask of
 * common/utils/misc.py:34-47 keeps keys < num_samp_hand).  Streaming-softmax (never
 * materialises Lq x Lk), exact fp32 on the f32 MFMA pipe; q is scaled by 1/sqrt(64).
 * o [B][Lq][ldo]; lse [B][H][Lq] = log2-domain log-sum-exp of the scaled scores (opaque,
 * only to be handed back to hoisdf_attention_bwd).
 * Dropout on the probabilities: mask of (b,h,i,j) is a hash of (seed, (b*H+h)*Lq+i, j). */
int hoisdf_attention_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                         float* o, int ldo, float* lse, int B, int H, int Lq, int Lk, int kv_len,
                         float drop_p, uint64_t seed, void* stream);
/* delta [B][H][Lq] is scratch. dq/dk/dv have the same layouts/ld as q/k/v. Rows of dk/dv at
 * keys >= kv_len are written as zero. */
int hoisdf_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                         const float* o, int ldo, const float* dout, int lddo, const float* lse,
                         float* delta, float* dq, float* dk, float* dv, int B, int H, int Lq, int Lk,
                         int kv_len, float drop_p, uint64_t seed, void* stream);
/* The 16-bit-operand evaluation attention on the pipelined forward (BASELINE.json configs[4], "fp16 MFMA attention"; what
 * cfg.attention_f16_eval selects):
 * Q, K, V and the probabilities as bf16 hi + lo pairs (two planes per operand: 16 significant bits, the f32 exponent range - none of
 * an f16 hi + lo scheme's power-of-two scaling, no overflow at trained sigma gates), three v_mfma_f32_32x32x16_bf16
 * products per product, f32 softmax state and accumulation.  Same layouts and kv_len semantics as hoisdf_attention_fwd; no dropout,
 * no lse.  reference: nn.MultiheadAttention forward inside the encoder layers (common/nets/transformer.py:269), BASELINE.json
 * configs[4].  workspace: hoisdf_attention_bf16x2_workspace(B, H, Lq, Lk) bytes, 16-byte aligned. */
long hoisdf_attention_bf16x2_workspace(int B, int H, int Lq, int Lk);
int hoisdf_attention_fwd_bf16x2(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                                int B, int H, int Lq, int Lk, int kv_len, void* workspace, long workspace_bytes, void* stream);

/* ---- fp32 attention emulated on the bf16 MFMA pipe ("bf16x3"; cfg.attention_emu, default) -------------------------------
 * reference: nn.MultiheadAttention inside the encoder layers (common/nets/transformer.py:269,286-302), forward + autograd
 * backward.  Same contracts, argument meaning, LSE convention (log2 domain) and dropout mask as hoisdf_attention_fwd / _bwd;
 * every contraction (QK^T, PV, dO V^T, dO^T P, Q^T dS, dS K) takes both f32 operands as exact bf16 triples and six bf16 MFMA
 * products per product with f32 accumulation (the arithmetic of hoisdf_linear_fwd_emu); softmax, dropout and the dS algebra stay
 * f32.  fp32-equivalent results (tests/test_gpu_emu.py), not bit-identical to the f32 entries.
 *   forward : workspace = hoisdf_attention_emu_workspace(B, H, Lq, Lk, keep ? 2 : 0) bytes, 16-byte aligned; keep = 1 leaves every
 *             Q / K / V plane the backward needs in it (pass it on as fwd_workspace).
 *   backward: ONE fused pass (dK, dV, dQ; 5 GEMM-equivalents), dQ through per-key-block partials summed in order - no atomics,
 *             run-to-run identical.  workspace = hoisdf_attention_bwd_emu_workspace(B, H, Lq, Lk, fwd_workspace != NULL) bytes.
 *             dq, dk, dv are fully overwritten (leading dimensions ldq, ldk, ldv of q, k, v). */
long hoisdf_attention_emu_workspace(int B, int H, int Lq, int Lk, int mode);
int hoisdf_attention_fwd_emu(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                             float* lse, int B, int H, int Lq, int Lk, int kv_len, float drop_p, uint64_t seed, void* workspace,
                             long workspace_bytes, int keep, void* stream);
/* the forward in the f16x2 form (round 5; see "the two arithmetic forms" at hoisdf_linear_fwd_emu_mag): q_mag / k_mag / v_mag = the head
 * magnitudes of q, k and v (each pointer positioned at ITS operand's first head: for q, k, v that are column slices 0 / E / 2E of one
 * [q | k | v] matrix with words w = hoisdf_head_mag_words(B L, 3 H, L): w, w + H B, w + 2 H B) - one power-of-two scale per (sample,
 * head) and operand (round 6; round 5 had one per matrix: a sample's rounding depended on its batch companions); two f16 planes per
 * operand, three v_mfma_f32_32x32x16_f16 products per product, P carried as 2^6 P.  Same contracts, LSE convention and dropout mask
 * as hoisdf_attention_fwd_emu; drop_p < 0.75.  Accuracy: the operand pieces keep 22 bits, so a score s (log2 domain) carries an
 * absolute error of ~2^-22 |s| where the bf16x3 form has f32 rounding only - indistinguishable at the |s| <~ 100 of trained attention,
 * 4x the bf16x3 form's output error at |s| ~ 2000.  The planes it keeps (keep = 1) are f16x2 planes - only a backward of the same form
 * reads them.  o_mag (optional, zero-filled, B Lq words) receives the row magnitudes of o. */
int hoisdf_attention_fwd_emu_mag(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                                 float* lse, int B, int H, int Lq, int Lk, int kv_len, float drop_p, uint64_t seed, void* workspace,
                                 long workspace_bytes, int keep, const uint32_t* q_mag, const uint32_t* k_mag, const uint32_t* v_mag,
                                 uint32_t* o_mag, void* stream);
long hoisdf_attention_bwd_emu_workspace(int B, int H, int Lq, int Lk, int kept);
int hoisdf_attention_bwd_emu(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, int ldo,
                             const float* dout, int lddo, const float* lse, float* delta, float* dq, float* dk, float* dv, int B,
                             int H, int Lq, int Lk, int kv_len, float drop_p, uint64_t seed, const void* fwd_workspace,
                             void* workspace, long workspace_bytes, void* stream);
/* the backward in the f16x2 form: Q, K, V, dO, P and dS as two scaled f16 pieces each (three products per product in all five
 * contractions, 60 instead of 120 MFMAs per query tile; emu_attn_bwd4g_kernel).  dS = Pd dP - P delta is scaled per (sample, head) by
 * the largest power of two sS with sS Bd (1 + 2^-10) < 2^14, where
 *     |dS_ij| <= Bd = inv_keep max_i ||dO_i||_2 8 max|V| + max_i |delta_i|
 * (Cauchy-Schwarz on dP_ij = dO_i . v_j over d = 64; the two maxima are by-products of the delta pass, max|V| is the head magnitude):
 * its two pieces carry the 22 bits of the other operands.  hoisdf_set_attn_bwd_ds(3) (environment HOISDF_ATTN_BWD_DS=3, read at first
 * use) brings back the earlier kernel for the calls that follow: a fixed dS scale from |dP| <= 64 max|dO| max|V|, which flat softmaxes
 * undershoot by ~20 binades, hence dS as THREE pieces (five products in dQ and dK, 76 MFMAs per query tile; emu_attn_bwd4h_kernel).
 * Either way one pass, no atomics, run-to-run identical like hoisdf_attention_bwd_emu.  q_mag / k_mag / v_mag: as hoisdf_attention_fwd_emu_mag; do_mag: the
 * head magnitudes of dout (all required; hoisdf_head_mag_measure, or hoisdf_linear_bwd_input_emu_heads).  fwd_workspace: the planes a
 * forward OF THIS FORM kept, or NULL.  g_mag (optional, zero-filled, B L words; needs Lq == Lk): the row magnitudes of a [dq | dk | dv] matrix. */
int hoisdf_attention_bwd_emu_mag(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, int ldo,
                                 const float* dout, int lddo, const float* lse, float* delta, float* dq, float* dk, float* dv, int B,
                                 int H, int Lq, int Lk, int kv_len, float drop_p, uint64_t seed, const void* fwd_workspace,
                                 void* workspace, long workspace_bytes, const uint32_t* q_mag, const uint32_t* k_mag,
                                 const uint32_t* v_mag, const uint32_t* do_mag, uint32_t* g_mag, void* stream);
/* the dS pieces of hoisdf_attention_bwd_emu_mag and of the layers that run it: 2 (default) or 3; process-wide, takes effect per call */
void hoisdf_set_attn_bwd_ds(int pieces);
int hoisdf_get_attn_bwd_ds(void);
/* Small masked attention (17 MANO queries, tgt_mask of common/utils/misc.py:11-31):
 * mask [Lq][Lk] uint8, 1 = masked; Lq, Lk <= 64. probs [B][H][Lq][Lk] saved for backward. */
int hoisdf_attention_small_fwd(const float* q, int ldq, const float* k, int ldk, const float* v,
                               int ldv, const uint8_t* mask, float* o, int ldo, float* probs, int B,
                               int H, int Lq, int Lk, float drop_p, uint64_t seed, void* stream);
int hoisdf_attention_small_bwd(const float* q, int ldq, const float* k, int ldk, const float* v,
                               int ldv, const float* probs, const float* dout, int lddo, float* dq,
                               float* dk, float* dv, int B, int H, int Lq, int Lk, float drop_p,
                               uint64_t seed, void* stream);

/* ---- residual + dropout + LayerNorm (common/nets/transformer.py:290-301) -----------------
 * y = LN(x + dropout(r)) * gamma + beta over rows of width D (D <= 1024, multiple of 4);
 * r may be NULL (plain LN, e.g. encoder.inter_norm / decoder.norm).  mean/rstd [M] saved. */
int hoisdf_add_layernorm_fwd(const float* x, const float* r, const float* gamma, const float* beta,
                             float* y, float* mean, float* rstd, long M, int D, float eps,
                             float drop_p, uint64_t seed, void* stream);
/* dx (gradient w.r.t. x), dr (w.r.t. r, may be NULL), dgamma/dbeta accumulated atomically. */
int hoisdf_add_layernorm_bwd(const float* dy, const float* x, const float* r, const float* gamma,
                             const float* mean, const float* rstd,
                             const float* dx_add /* optional [M][D]: added into dx (another consumer's gradient) */,
                             float* dx, float* dr, float* dgamma, float* dbeta, long M, int D, float drop_p,
                             uint64_t seed, void* stream);

/* y = x + dropout(r) over rows of width D (multiple of 4) - the residual of a PRE-norm layer (reference
 * common/nets/transformer.py:304-331 TransformerEncoderLayer.forward_pre, :397-437 TransformerDecoderLayer.forward_pre; main/config.py:122
 * cfg.pre_norm).  x == NULL: y = dropout(r), which is also the backward (dr = dropout-mask(dy) with the SAME seed; dx = dy).
 * The mask is the (seed, row, column) function of hoisdf_add_layernorm_fwd.  Buffers 16-byte aligned; y may alias r. */
int hoisdf_residual_dropout(const float* x, const float* r, float* y, long M, int D, float drop_p, uint64_t seed, void* stream);

/* Plain LayerNorm of the FIRST `take` rows of every group of `rows_per_group` input rows (the encoder stack's inter_norm:
 * main/model.py:587-593 only ever reads the hand / object rows of each layer's normalised output).  x [groups *
 * rows_per_group][D]; y, mean, rstd compact [groups * take].  Backward: dy compact; dx covers ALL input rows - rows that
 * were normalised get their LayerNorm gradient (+ dx_add), the others dx_add (or 0 when dx_add is NULL). */
int hoisdf_layernorm_rows_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                              long groups, int rows_per_group, int take, int D, float eps, void* stream);
int hoisdf_layernorm_rows_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                              const float* dx_add, float* dx, float* dgamma, float* dbeta, long groups, int rows_per_group,
                              int take, int D, void* stream);

/* ---- one transformer encoder layer per call (SURVEY.md section 8(b) coarse entries) ---------------------------------
 * reference: common/nets/transformer.py:286-302 (TransformerEncoderLayer.forward_post: self-attention, out-projection,
 * residual + dropout + LayerNorm, FFN linear1 -> ReLU -> dropout -> linear2, residual + dropout + LayerNorm) and the
 * stack's inter_norm of each layer output (:117-131).  Host-side chains of the per-op entries above on the caller's stream.
 * x [B][S][E] (dense).  Rows < n_query of every sample are produced: x_out [B][n_query][E]; with weights.g3 the
 * inter_norm of rows < n_inter goes to y_out [B][n_inter][E].  Keys / values always come from all S rows.
 * Arithmetic: linear layers follow hoisdf_set_gemm_emu (default: fp32 emulated on the bf16 pipe from 2048 rows up; the
 * img_* fields may carry hoisdf_linear_emu_prepare images of the weights (img_t_*: transpose = 1) - a NULL image is built
 * in the workspace on every call); attention as desc.attention says.  Split-precision / f16 modes are not offered here.
 * saved: hoisdf_encoder_layer_saved_bytes(desc) bytes the backward re-reads (training = 1); workspace:
 * hoisdf_encoder_layer_workspace_bytes(desc, 0 | 1) bytes of scratch (sized for the case that every image is built).
 * Backward: g_x_out / g_y = gradients of the two outputs (either may be NULL, not both); dx [B][S][E] is overwritten; the
 * parameter gradients must be zero on entry and hold the gradient on return. */
typedef struct hoisdf_encoder_layer_desc {
  int B, S, E, F, H;            /* batch, tokens per sample, model width (multiple of 4 and of H), FFN width, heads */
  int n_query;                  /* <= 0 or >= S: all rows */
  int n_inter;                  /* <= 0 or >= n_query: all produced rows */
  float eps, drop_p;
  uint64_t seed[4];             /* dropout streams: attention, after out-projection, FFN hidden, after the FFN */
  int attention;                /* 0: exact-f32 kernels; 2: emulated-fp32 forward (hoisdf_attention_fwd_emu) */
  int attention_bwd_emulated;   /* with attention == 2: the order-fixed emulated backward instead of the f32 fused one */
  int training;                 /* 0: nothing is saved (saved may be NULL), hoisdf_encoder_layer_bwd cannot follow */
  const uint32_t* x_mag;        /* optional: row magnitudes of x (B S words; f16x2 form, see hoisdf_linear_fwd_emu_mag; NULL = the layer
                                 * measures x itself), e.g. hoisdf_encoder_layer_out_mag of the layer below; must stay valid until the backward */
} hoisdf_encoder_layer_desc;
/* where a training forward left the row magnitudes of x_out (B n_query words) inside `saved` (NULL when the layer's contractions do
 * not run in the f16x2 form): the x_mag of the next layer's descriptor */
const uint32_t* hoisdf_encoder_layer_out_mag(const hoisdf_encoder_layer_desc* d, const void* saved);
typedef struct hoisdf_encoder_layer_weights {
  const float *w_in, *b_in;     /* [3E][E], [3E]: packed q | k | v in-projection */
  const float *w_out, *b_out;   /* [E][E], [E] */
  const float *g1, *be1;        /* norm1 */
  const float *w1, *b1;         /* [F][E], [F] */
  const float *w2, *b2;         /* [E][F], [E] */
  const float *g2, *be2;        /* norm2 */
  const float *g3, *be3;        /* inter_norm of the stack; NULL: no y_out */
  const void *img_in, *img_in_q, *img_in_kv, *img_out, *img_1, *img_2;              /* optional (see above); _q = rows [0, E), _kv = rows [E, 3E) */
  const void *img_t_in, *img_t_in_q, *img_t_in_kv, *img_t_out, *img_t_1, *img_t_2;
} hoisdf_encoder_layer_weights;
typedef struct hoisdf_encoder_layer_grads {
  float *dw_in, *db_in, *dw_out, *db_out, *dg1, *dbe1, *dw1, *db1, *dw2, *db2, *dg2, *dbe2, *dg3, *dbe3;
} hoisdf_encoder_layer_grads;
long hoisdf_encoder_layer_saved_bytes(const hoisdf_encoder_layer_desc* desc);
long hoisdf_encoder_layer_workspace_bytes(const hoisdf_encoder_layer_desc* desc, int backward_pass);
int hoisdf_encoder_layer_fwd(const float* x, const hoisdf_encoder_layer_weights* weights, const hoisdf_encoder_layer_desc* desc,
                             float* x_out, float* y_out, void* saved, long saved_bytes, void* workspace, long workspace_bytes,
                             void* stream);
int hoisdf_encoder_layer_bwd(const float* x, const float* x_out, const hoisdf_encoder_layer_weights* weights,
                             const hoisdf_encoder_layer_desc* desc, const void* saved, long saved_bytes, const float* g_x_out,
                             const float* g_y, float* dx, const hoisdf_encoder_layer_grads* grads, void* workspace,
                             long workspace_bytes, void* stream);

/* ---- one transformer decoder layer per call ---------------------------------------------------------------------------
 * reference: common/nets/transformer.py:366-395 (TransformerDecoderLayer.forward_post) as the hand stack runs it, and the
 * decoder stack's norm of every layer output (:150-163).  tgt [B][Q][E] (Q <= 64 MANO queries), memory [B][S][E] (the encoder
 * output; only keys < kv_len are attended = the memory mask of common/utils/misc.py:34-47), query_pos [Q][E] (broadcast over
 * the batch, added to the queries / keys of the self-attention and the queries of the cross-attention), tgt_mask [Q][Q]
 * uint8 (1 = masked).  out [B][Q][E]; with weights.g4, y_out = the stack norm of out.  Buffers and arithmetic as for the
 * encoder layer (the 17-query attention kernels are exact f32; the memory's K / V projection follows hoisdf_set_gemm_emu).
 * Backward: d_tgt is overwritten; d_memory is overwritten or (accumulate_memory = 1: the memory feeds every decoder layer)
 * added to; d_query_pos [Q][E] (may be NULL) is ADDED to; parameter gradients zero on entry. */
typedef struct hoisdf_decoder_layer_desc {
  int B, Q, S, E, F, H, kv_len;
  float eps, drop_p;
  uint64_t seed[6];             /* dropout streams: self-attention, after its out-projection, cross-attention, after its
                                   out-projection, FFN hidden, after the FFN */
  int training;
} hoisdf_decoder_layer_desc;
typedef struct hoisdf_decoder_layer_weights {
  const float *sa_w_in, *sa_b_in, *sa_w_out, *sa_b_out;      /* self_attn: [3E][E], [3E], [E][E], [E] */
  const float *ca_w_in, *ca_b_in, *ca_w_out, *ca_b_out;      /* multihead_attn */
  const float *w1, *b1, *w2, *b2;                            /* [F][E], [F], [E][F], [E] */
  const float *g1, *be1, *g2, *be2, *g3, *be3;               /* norm1..3 */
  const float *g4, *be4;                                     /* the stack's norm; NULL: no y_out */
  const void *img_ca_kv, *img_t_ca_kv;                       /* optional bf16x3 images of ca_w_in rows [E, 3E) (and transposed) */
} hoisdf_decoder_layer_weights;
typedef struct hoisdf_decoder_layer_grads {
  float *dsa_w_in, *dsa_b_in, *dsa_w_out, *dsa_b_out, *dca_w_in, *dca_b_in, *dca_w_out, *dca_b_out, *dw1, *db1, *dw2, *db2,
      *dg1, *dbe1, *dg2, *dbe2, *dg3, *dbe3, *dg4, *dbe4;
} hoisdf_decoder_layer_grads;
long hoisdf_decoder_layer_saved_bytes(const hoisdf_decoder_layer_desc* desc);
long hoisdf_decoder_layer_workspace_bytes(const hoisdf_decoder_layer_desc* desc, int backward_pass);
int hoisdf_decoder_layer_fwd(const float* tgt, const float* memory, const float* query_pos, const uint8_t* tgt_mask,
                             const hoisdf_decoder_layer_weights* weights, const hoisdf_decoder_layer_desc* desc, float* out,
                             float* y_out, void* saved, long saved_bytes, void* workspace, long workspace_bytes, void* stream);
int hoisdf_decoder_layer_bwd(const float* tgt, const float* memory, const uint8_t* tgt_mask, const float* out,
                             const hoisdf_decoder_layer_weights* weights, const hoisdf_decoder_layer_desc* desc, const void* saved,
                             long saved_bytes, const float* g_out, const float* g_y, float* d_tgt, float* d_memory,
                             int accumulate_memory, float* d_query_pos, const hoisdf_decoder_layer_grads* grads, void* workspace,
                             long workspace_bytes, void* stream);

/* ---- K12: vote aggregation ----------------------------------------------------------------
 * reference: common/nets/loss.py:31-56.  off [L][B][P][J*3], cls [L][B][P][J] (batch-first
 * rows), pts [B][P][3].  joints[l][b][j] = sum_p softmax_p(cls)[p] * (pts[p] + off[p][j]).
 * stats [L][B][J][2] = (max, sum of exp) of each softmax column, saved for the backward. */
int hoisdf_vote_fwd(const float* off, const float* cls, const float* pts, float* joints, float* stats,
                    int L, int B, int P, int J, void* stream);
int hoisdf_vote_bwd(const float* off, const float* cls, const float* pts, const float* joints,
                    const float* stats, const float* djoints, float* doff, float* dcls, int L, int B,
                    int P, int J, void* stream);

/* K12 with the three JointvoteLoss reductions fused (common/nets/loss.py:31-56): besides joints / stats
 * (as hoisdf_vote_fwd) one pass writes, per (l, b):
 *   l3d_sum [L][B] = sum_{p,j,d} smooth_l1(1000*(pts+off) - gt_mm) * near,   near = ||pts - gt_mm/1000|| < radius
 *   bce_sum [L][B] = sum_{p,j} binary_cross_entropy_with_logits(cls, near);  near_sum [B] = sum_{p,j} near.
 * The reference's scalars are loss_joint_3d = mean_l(sum_b l3d_sum / sum_b near_sum) / 3,
 * loss_joint_cls = sum(bce_sum) / (L*B*P*J).  The backward takes d(loss)/d(l3d_sum), d/d(bce_sum) [L][B]
 * and d/d(joints) [L][B][J][3] (any of them may be NULL = zero). */
int hoisdf_vote_loss_fwd(const float* off, const float* cls, const float* pts, const float* joint_gt_mm,
                         float radius, float* joints, float* stats, float* l3d_sum, float* bce_sum,
                         float* near_sum, int L, int B, int P, int J, void* stream);
int hoisdf_vote_loss_bwd(const float* off, const float* cls, const float* pts, const float* joint_gt_mm,
                         float radius, const float* joints, const float* stats, const float* djoints,
                         const float* dl3d_sum, const float* dbce_sum, float* doff, float* dcls, int L,
                         int B, int P, int J, void* stream);

/* ---- K1 + K7 + K8 and K11 + K12 as single calls (SURVEY.md section 8(b) `hoisdf_token_build_*`, `hoisdf_heads_vote_*`) ----------
 * An MLP = Linear (+ ReLU) chain as common/nets/layer.py:168-201 builds it: layer i maps dims[i] -> dims[i + 1] with weight
 * w[i] [dims[i + 1]][dims[i]] (dense) and bias b[i]; ReLU after every layer but the last, and after the last one too when
 * act_last (linear_transformerin, main/model.py:58-62).  Gradient buffers are zero on entry and hold the gradient on return.
 *
 * hoisdf_tokens_fwd: the token rows of one point set (reference: Model.get_input_transformer, main/model.py:145-179, + the
 *   sigma gate and concatenation, :123-126,520-562): feat [B P][C] = the gathered pyramid rows (feat_in with their camera points
 *   cam_in [B P][3]; or feat_in = NULL: projected + gathered here from pyr / points [B][P][3] / cam_intr, cam_out [B P][3]
 *   receives the camera points) -> MLP -> fea [B P][D - 33] -> tok[b][row0 + p][:] = [cam - center | pe | fea * sigmoid(sdf /
 *   beta) / beta] (hoisdf_token_build_fwd).  fea_out (optional) receives the MLP output for other consumers (the detached
 *   cross-field tokens, :540,:558).  hoisdf_tokens_bwd: dtok [B][S][D] -> the MLP's weight gradients, *dbeta += ..., and the
 *   gradient of the gathered rows into dfeat [B P][C] (overwritten or, accumulate_dfeat = 1, added to) - or, when the rows were
 *   gathered inside and dpyr is given, scatter-added into the pyramid gradient.
 * hoisdf_heads_vote_fwd: enc [L][B][P][E] = the intermediate hand rows of all L encoder depths (main/model.py:587-593) ->
 *   linear_handvote / linear_handcls -> hoisdf_vote_loss_fwd: joints [L][B][J][3] and the three reductions of
 *   JointvoteLoss (see hoisdf_vote_loss_fwd).  hoisdf_heads_vote_bwd: gradients of joints / l3d_sum / bce_sum (any may be NULL)
 *   -> both MLPs' weight gradients and denc [L B P][E] (overwritten). */
#define HOISDF_MLP_MAX_LAYERS 4
typedef struct hoisdf_mlp {
  int n_layers, act_last;
  int dims[HOISDF_MLP_MAX_LAYERS + 1];
  const float* w[HOISDF_MLP_MAX_LAYERS];
  const float* b[HOISDF_MLP_MAX_LAYERS];
  /* optional (NULL = built per call in the workspace): the bf16x3 slab images of w[i] (hoisdf_linear_emu_prepare, transpose 0 for
   * the forward, transpose 1 for the grad-input GEMM) when the caller keeps them cached across calls - a training step otherwise
   * rebuilds ~30 of them inside these entries */
  const void* img[HOISDF_MLP_MAX_LAYERS];
  const void* img_t[HOISDF_MLP_MAX_LAYERS];
} hoisdf_mlp;
typedef struct hoisdf_mlp_grads {
  float* dw[HOISDF_MLP_MAX_LAYERS];
  float* db[HOISDF_MLP_MAX_LAYERS];
} hoisdf_mlp_grads;
long hoisdf_tokens_saved_bytes(const hoisdf_mlp* mlp, long n_rows, int gather_inside);
long hoisdf_tokens_workspace_bytes(const hoisdf_mlp* mlp, long n_rows, int backward_pass);
int hoisdf_tokens_fwd(const hoisdf_pyramid* pyr, const float* points, const float* center, const float* cam_intr, float scale,
                      int img_h, int img_w, const float* feat_in, const float* cam_in, const hoisdf_mlp* mlp, const float* pe,
                      const float* sdf, const float* beta_ptr, float* tok, float* fea_out, float* cam_out, int B, int P, int S,
                      int row0, int D, void* saved, long saved_bytes, void* workspace, long workspace_bytes, void* stream);
int hoisdf_tokens_bwd(const hoisdf_pyramid_grad* dpyr, const float* points, const float* center, const float* cam_intr,
                      float scale, int img_h, int img_w, const float* feat_in, const hoisdf_mlp* mlp, const float* sdf,
                      const float* beta_ptr, const float* dtok, const void* saved, long saved_bytes,
                      const hoisdf_mlp_grads* grads, float* dfeat, int accumulate_dfeat, float* dbeta, int B, int P, int S,
                      int row0, int D, void* workspace, long workspace_bytes, void* stream);
long hoisdf_heads_vote_saved_bytes(const hoisdf_mlp* vote, const hoisdf_mlp* cls, int L, int B, int P, int J);
long hoisdf_heads_vote_workspace_bytes(const hoisdf_mlp* vote, const hoisdf_mlp* cls, int L, int B, int P, int J,
                                       int backward_pass);
int hoisdf_heads_vote_fwd(const float* enc, const hoisdf_mlp* vote, const hoisdf_mlp* cls, const float* pts,
                          const float* joint_gt_mm, float radius, float* joints, float* l3d_sum, float* bce_sum,
                          float* near_sum, int L, int B, int P, int J, void* saved, long saved_bytes, void* workspace,
                          long workspace_bytes, void* stream);
int hoisdf_heads_vote_bwd(const float* enc, const hoisdf_mlp* vote, const hoisdf_mlp* cls, const float* pts,
                          const float* joint_gt_mm, float radius, const float* joints, const void* saved, long saved_bytes,
                          const float* djoints, const float* dl3d_sum, const float* dbce_sum,
                          const hoisdf_mlp_grads* vote_grads, const hoisdf_mlp_grads* cls_grads, float* denc, int L, int B,
                          int P, int J, void* workspace, long workspace_bytes, void* stream);

/* ---- a15: the scalar point losses ------------------------------------------------
 * reference: common/nets/loss.py:64-78 (SepSDFLoss = torch.nn.L1Loss(mean) of the clamped SDF predictions against the
 * ground truth clamped as main/model.py:393-400 does), main/model.py:35-36,656-662 (obj_rot / obj_trans:
 * torch.nn.SmoothL1Loss, beta 1, mean over (L, B, P, 3) against the (B, 3) target expanded over depth and points),
 * common/nets/loss.py:57-59 (loss_all_joint_3d: SmoothL1 of joints * 1000 against the ground truth expanded over depth).
 * Element i of pred [n] is compared with target[((i / (rep * C)) % Bt) * C + i % C] - a (Bt, C) target broadcast over
 * leading dimensions and over `rep` repeats between Bt and C.  kind 0: |pred * pred_scale - clamp(target, +-clamp)|
 * (clamp <= 0: the target is taken as is); kind 1: SmoothL1 with beta = 1 of the same difference.
 * fwd: loss[0] = out_scale * sum_i (out_scale = 1 / n gives the reference's mean); order-fixed (per-block partial sums in
 *   partials [hoisdf_point_loss_blocks(n)] added in block order): bit-reproducible.
 * bwd: dpred[i] = g[0] * out_scale * pred_scale * dl/dd (torch's subgradients: sign(0) = 0). */
int hoisdf_point_loss_blocks(long n);
int hoisdf_point_loss_fwd(const float* pred, const float* target, long n, long rep, int C, long Bt, int kind,
                          float clamp, float pred_scale, float out_scale, float* partials, float* loss, void* stream);
int hoisdf_point_loss_bwd(const float* pred, const float* target, long n, long rep, int C, long Bt, int kind,
                          float clamp, float pred_scale, float out_scale, const float* g, float* dpred, void* stream);

/* ---- (f3) MANO head ---------------------------------------------------------------------------------------------
 * reference: common/nets/mano_head.py:12-278 (6D -> rotation -> quaternion -> axis-angle, the head), manopth/manopth/
 * manolayer.py:111-276 (the layer as main/model.py:735-742 configures it: use_pca=False, flat_hand_mean=True,
 * center_idx=0, side right), common/nets/loss.py:81-171 (ManoLoss: four MSE terms).  One workgroup per hand.
 *
 * hoisdf_mano_prepare: the layer's blend-shape tables th_shapedirs [778][3][10] and th_posedirs [778][3][135] transposed
 *   into one image [145][2334], followed by th_weights [778][16] transposed (hoisdf_mano_dirs_image_floats() floats in
 *   all) - build it once per set of assets.
 * hoisdf_mano_head_fwd, for `hands` hands:
 *   mode 0 (predictions): pose = 6D rotations [hands][16][6] (row stride ldpose >= 96), betas [hands][>= 10];
 *   mode 1 (ground truth): pose = axis-angle MANO coefficients [hands][>= 48] as the dataset stores them (mano_param[:, :48]:
 *     the head subtracts hands_mean from [3:48] and the layer adds it back; rot = Rodrigues of the mean-free coefficients);
 *   v_template [778][3], j_regressor [16][778], weights [778][16] (16-byte aligned), hands_mean [45];
 *   outputs in metres, centred on the wrist: verts [hands][778][3], joints [hands][21][3] (the reference's 21-joint order),
 *   rot [hands][16][3][3] (mode 0: the Gram-Schmidt rotations = pred mano_pose).
 *   With gt_verts != NULL (mode 0) hand h is compared with ground-truth hand h % gt_hands and
 *   loss_sums [hands][4] = sum of squared errors of (verts, joints, rot, betas) - the reference's four ManoLoss terms are
 *   lambda_i * sum_h loss_sums[h][i] / (hands * {2334, 63, 144, 10}).
 * hoisdf_mano_head_bwd (mode 0 inputs again; nothing is saved between the calls): upstream gradients g_loss_sums
 *   [hands][4], g_verts, g_joints, g_rot (each may be NULL = zero) -> d_pose6d [hands][16][6], d_betas [hands][10].
 *   hands_mean must be zero (flat_hand_mean=True): the backward applies the layer's rotation gradient to the 6D rotation
 *   directly, which is exact only then (csrc/mano.hip header).
 * hoisdf_ik_mano_fwd: the closed-form inverse kinematics of the IK variant (common/utils/inverse_kinematics.py:15-150 as
 *   main/test.py:139-160 applies it) and the MANO layer on its result, ONE launch for `hands` hands (hands mean zero):
 *   joints with n_joints = 21: [hands][21][3] metres, wrist in row 0 at any translation; n_joints = 20: [hands][20][3] = joints
 *   1..20 relative to a wrist at the origin (the layout of hoisdf_pose_outputs.hand_joints_out); betas [hands][>= 10] with row
 *   stride ldbetas, NULL = zeros.  The palm fit (Kabsch over the five palm bones) is a proper rotation or a reflection:
 *   valid_out [hands] (may be NULL) = 1 / 0, and a reflected hand keeps the zero pose.  A SINGULAR fit (all-zero joints, exactly
 *   coplanar palm bones: rank < 3) takes the identity as the palm rotation with valid = 1, where an SVD would return one of the
 *   equally good rotations - degenerate input, not a case either solver answers meaningfully.  pose_out [hands][48] axis-angle,
 *   verts_out [hands][778][3] and joints_out [hands][21][3] in metres at the input wrist.  No atomics: two calls, same bits. */
long hoisdf_mano_dirs_image_floats(void);
int hoisdf_mano_prepare(const float* shapedirs, const float* posedirs, const float* weights, float* image, void* stream);
int hoisdf_mano_head_fwd(const float* pose, int ldpose, int mode, const float* betas, int ldbetas, int hands,
                         const float* dirs_image, const float* v_template, const float* j_regressor, const float* weights,
                         const float* hands_mean, const float* gt_verts, const float* gt_joints, const float* gt_rot,
                         const float* gt_shape, int ldgt_shape, int gt_hands, float* verts, float* joints, float* rot,
                         float* loss_sums, void* stream);
int hoisdf_mano_head_bwd(const float* pose6d, const float* betas, int hands, const float* dirs_image, const float* v_template,
                         const float* j_regressor, const float* weights, const float* hands_mean, const float* gt_verts,
                         const float* gt_joints, const float* gt_rot, const float* gt_shape, int ldgt_shape, int gt_hands,
                         const float* g_loss_sums, const float* g_verts, const float* g_joints, const float* g_rot,
                         float* d_pose6d, float* d_betas, void* stream);
int hoisdf_ik_mano_fwd(const float* joints, int n_joints, const float* betas, int ldbetas, int hands,
                       const float* dirs_image, const float* v_template, const float* j_regressor, const float* weights,
                       float* pose_out, float* verts_out, float* joints_out, int32_t* valid_out, void* stream);

/* ---- whole-model inference: the stage after the image encoder as ONE entry ---------------------------------------------
 * reference: the eval forward of Model.forward behind decoder_net (main/model.py:424-662, the sdf_infer branch :462-481): feature
 * pyramid + camera inputs + boxes in, hand joints / object pose / MANO mesh out.  No losses, no targets, dropout off.  The host
 * composite (csrc/pose_infer.hip) issues the coarse entries above in the order hoisdf_amd/model.py Model.hot_path does, so the
 * same shape takes the same kernel on either host; only what inference reads is computed (heads and stack norms on the LAST
 * layer's rows only).  Call sequence of a host (INTEGRATION.md "the whole pose stage from C"):
 *   once   : hoisdf_pose_prepared_bytes -> allocate -> hoisdf_pose_prepare (everything that depends on the weights alone: copies of
 *            the parameters, the weight-norm folds of both SDF decoders in the layouts of hoisdf_sdf_weights, the weight images of
 *            the emulated GEMMs in the process's form, the MANO table image, both sigmoid_beta floored at 2e-3, the MANO target
 *            mask, the zero decoder input).  The blob is self-contained: the caller's weight buffers may go once the stream has
 *            executed the call.  Rebuild it when a weight changes.
 *   frame  : hoisdf_pose_infer_begin (queues both survivor counts, returns without waiting: issue it ahead of the image encoder)
 *            -> wait until `stream` has executed it -> hoisdf_pose_infer_workspace(desc, counts_host) -> hoisdf_pose_infer.
 * The 2 B survivor counts are the one device -> host read of the path (counts [0, B) = hand field, [B, 2 B) = object field;
 * counts_host is page-locked host memory). */
typedef struct hoisdf_pose_desc {
  int B;                           /* samples */
  int num_samp_hand, num_samp_obj; /* query points per field (cfg.num_samp_hand / num_samp_obj) */
  int bins_n;                      /* lattice resolution of sdf_infer (cfg.bins_n) */
  int img_h, img_w;                /* cfg.input_img_shape */
  float hand_sdf_scale, obj_sdf_scale, clamping_distance;   /* cfg.hand_sdf_scale / obj_sdf_scale / ClampingDistance */
  int hidden_dim;                  /* 256: the SDF decoders and the token layout [3 | 30 | 223] are built for it */
  int nheads;                      /* hidden_dim / 64 (the attention kernels hold heads of 64) */
  int dim_feedforward;
  int enc_layers;                  /* hand encoder depth; the object encoder has enc_layers / 2 (main/model.py:712-720) */
  int dec_layers;
  int C;                           /* pyramid channels (992 / 3968) */
  int use_inverse_kinematics;      /* 1: one decoder query, mano_shape_out only, no MANO head (main/model.py:595-597) */
  int pre_norm;                    /* cfg.pre_norm: refused (the coarse layer entries are post-norm) */
  int classifier_branch;           /* cfg.ClassifierBranch: the class logits are read by nothing in this path; accepted, no effect */
  int attention;                   /* 0: exact-f32 attention kernels; 2: emulated fp32 (the default of hoisdf_encoder_layer_desc) */
  int ik_solve;                    /* with use_inverse_kinematics only: 1 = hoisdf_ik_mano_fwd on hand_joints_out + mano_shape_out as the
                                      call's last launch -> mano_pose_out, mano_mesh_out, mano_joints_out (the MANO assets become required) */
} hoisdf_pose_desc;
#define HOISDF_POSE_MAX_LAYERS 12
/* hand_sdf_decoder.* / obj_sdf_decoder.* as checkpointed (torch weight_norm, legacy naming) */
typedef struct hoisdf_sdf_decoder_params {
  const float* weight_v[4];        /* linh0 .. linh3: [512][289], [223][512], [512][512], [512][512] */
  const float* weight_g[4];        /* [512], [223], [512], [512] */
  const float* bias[4];
  const float *linh4_weight, *linh4_bias;   /* [1][512], [1] */
} hoisdf_sdf_decoder_params;
/* One pointer per parameter of the path, named after the checkpoint keys (tests/golden/g10_state_dict_schema.json).  Image fields of
 * the member structs are ignored (the prepared blob carries its own). */
typedef struct hoisdf_pose_weights {
  hoisdf_mlp linear_sdfin;                 /* C -> 512 -> 256, ReLU after both */
  hoisdf_sdf_decoder_params hand_sdf_decoder, obj_sdf_decoder;
  hoisdf_mlp linear_transformerin;         /* C -> 1024 -> 512 -> 256 -> hidden_dim - 33, ReLU after all four */
  const float *hand_sigmoid_beta, *obj_sigmoid_beta;        /* [1] each */
  hoisdf_encoder_layer_weights hand_encoder[HOISDF_POSE_MAX_LAYERS];   /* hand_transformer.encoder.layers.i; g3 / be3 = encoder.inter_norm */
  hoisdf_encoder_layer_weights obj_encoder[HOISDF_POSE_MAX_LAYERS];    /* obj_transformer.encoder.layers.i (enc_layers / 2 of them) */
  hoisdf_decoder_layer_weights hand_decoder[HOISDF_POSE_MAX_LAYERS];   /* hand_transformer.decoder.layers.i; g4 / be4 = decoder.norm */
  const float* mano_query_embed;           /* [17][hidden_dim], or [1][hidden_dim] with use_inverse_kinematics */
  hoisdf_mlp linear_pose;                  /* hidden -> hidden -> hidden -> 6 (unused with use_inverse_kinematics) */
  hoisdf_mlp linear_shape;                 /* hidden -> hidden -> hidden -> 10 */
  hoisdf_mlp linear_handvote;              /* hidden -> hidden -> hidden -> hidden -> 60 */
  hoisdf_mlp linear_handcls;               /* hidden -> hidden -> hidden -> 20 */
  hoisdf_mlp linear_obj_rot;               /* hidden -> hidden -> hidden -> 3 */
  hoisdf_mlp linear_obj_rel_trans;         /* hidden -> hidden -> hidden -> 3 */
  /* MANO assets (unused with use_inverse_kinematics unless ik_solve): what hoisdf_mano_prepare / hoisdf_mano_head_fwd take; hands_mean must be
   * zero.  With ik_solve mano_hands_mean is NOT read (may be NULL): hoisdf_ik_mano_fwd solves for a layer with a zero hand mean
   * (flat_hand_mean=True), and a host whose layer has another mean must not use it */
  const float *mano_shapedirs, *mano_posedirs, *mano_weights, *mano_v_template, *mano_j_regressor, *mano_hands_mean;
} hoisdf_pose_weights;
typedef struct hoisdf_pose_outputs {
  float* hand_joints_out;          /* [B][20][3] */
  float* obj_rot_out;              /* [B][num_samp_obj][3] */
  float* obj_trans_out;            /* [B][num_samp_obj][3] */
  float* mano_mesh_out;            /* [B][778][3]  (with use_inverse_kinematics: only with ik_solve, the IK result, wrist at the origin) */
  float* mano_joints_out;          /* [B][21][3]   (the same) */
  float* mano_shape_out;           /* [B][10]      (use_inverse_kinematics only) */
  /* optional debug outputs (NULL = skipped): the selected points (scaled SDF frame) and their clamped SDF values */
  float *hand_points_out, *obj_points_out;   /* [B][num_samp_*][3] */
  float *hand_sdf_out, *obj_sdf_out;         /* [B][num_samp_*] */
  /* ik_solve only */
  float* mano_pose_out;            /* [B][48] axis-angle MANO coefficients */
  int32_t* ik_valid_out;           /* [B], optional: 1 = the palm fit is a proper rotation, 0 = a reflection (pose left at zero) */
} hoisdf_pose_outputs;
long hoisdf_pose_prepared_bytes(const hoisdf_pose_desc* desc);
int hoisdf_pose_prepare(const hoisdf_pose_desc* desc, const hoisdf_pose_weights* weights, void* prepared, long prepared_bytes,
                        void* stream);
int hoisdf_pose_infer_begin(const hoisdf_pose_desc* desc, const float* center_hand, const float* center_obj, const float* cam_intr,
                            const float* bbox_hand, const float* bbox_obj, int32_t* counts_device, int32_t* counts_host,
                            void* stream);
long hoisdf_pose_infer_workspace(const hoisdf_pose_desc* desc, const int32_t* counts_host);
/* Only enqueues.  side_stream == NULL: everything on `stream`; otherwise the object-point work, the object encoder stack with its
 * heads and the MANO head go to side_stream, forked and joined with events as hoisdf_amd/model.py does, and the call returns with
 * `stream` ordered behind all of it.  The results do not depend on side_stream.  A sample with fewer survivors than requested
 * points is refused (HOISDF_ERR_TOO_FEW) before anything is launched.  prepared / workspace: 256-byte aligned device memory. */
int hoisdf_pose_infer(const hoisdf_pose_desc* desc, const void* prepared, const hoisdf_pyramid* pyr, const float* center_hand,
                      const float* center_obj, const float* cam_intr, const float* bbox_hand, const float* bbox_obj,
                      const int32_t* counts_device, const int32_t* counts_host, const hoisdf_pose_outputs* outputs,
                      void* workspace, long workspace_bytes, void* side_stream, void* stream);

/* ---- convolution forward on channels-last maps (csrc/conv.hip): exact f32, evaluation only ------------------------------------
 * reference: torch.nn.functional.conv2d / conv_transpose2d / max_pool2d as common/nets/resnet.py and common/nets/layer.py use them.
 * An implicit GEMM on the f32 MFMA pipe (bit-for-bit an fmaf chain): output row m = (b, oy, ox), contraction k = (ky, kx, ci).
 * x: dense NHWC map [B][H][W][C_in] with a row stride ldx >= C_in (a channel slice of a wider map works).  Weights are packed once
 * by hoisdf_conv_pack_weight (hoisdf_conv_packed_floats floats + a bias of C_out rounded up to 4 floats; packed 16-byte aligned),
 * which also folds an evaluation-mode BatchNorm: gamma != NULL -> s = gamma / sqrt(var + eps) (f64, rounded once), w' = w s,
 * b' = (conv_bias - mean) s + beta.  w is torch's [C_out][C_in][KH][KW], or with transposed = 1 ConvTranspose2d's [C_in][C_out][4][4].
 * Epilogue: y[pixel][c_off + co] = act(acc + bias[co] (+ residual[pixel][co])), y row stride ldy >= c_off + C_out, residual row stride
 * ldr; act 0 none / 1 ReLU / 2 sigmoid.  hoisdf_conv_transpose2d_fwd is ConvTranspose2d(4, 2, 1): x is [B][H][W][C_in], y the
 * [B][2 H][2 W] map, computed as its four output-parity classes (2x2-tap convolutions, K = 4 C_in).
 * A problem of few output tiles cuts K over workgroups (hoisdf_conv_plan: tile 64 / 128, splitk > 1) through partial tiles in the
 * caller's workspace and an ordered reduce - no float atomics, two runs give the same bits; hoisdf_conv_workspace_bytes(M, C_out, K,
 * classes) with M = output rows (B OH OW; transposed: B H W), K = KH KW C_in (transposed: 4 C_in), classes = 1 (transposed: 4).
 * hoisdf_maxpool2d_fwd: MaxPool2d(3, 2, 1), y = [B][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]. */
long hoisdf_conv_packed_floats(int C_out, int C_in, int KH, int KW);
int hoisdf_conv_pack_weight(const float* w, const float* conv_bias, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, int C_out, int C_in, int KH, int KW, int transposed, float* packed,
                            float* bias_out, void* stream);
int hoisdf_conv_plan(long M, int C_out, int K, int classes, int* tile, int* splitk);
long hoisdf_conv_workspace_bytes(long M, int C_out, int K, int classes);
int hoisdf_conv2d_fwd(const float* x, int ldx, const float* w_packed, const float* bias, const float* residual, int ldr, float* y,
                      int ldy, int c_off, int B, int H, int W, int C_in, int C_out, int KH, int KW, int stride, int pad, int act,
                      void* workspace, long workspace_bytes, void* stream);
int hoisdf_conv_transpose2d_fwd(const float* x, int ldx, const float* w_packed, const float* bias, float* y, int ldy, int c_off, int B,
                                int H, int W, int C_in, int C_out, int act, void* workspace, long workspace_bytes, void* stream);
int hoisdf_maxpool2d_fwd(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, void* stream);

/* ---- the image encoder in evaluation mode: image -> feature pyramid (csrc/encoder_infer.hip) ---------------------------------
 * reference: backbone_net + decoder_net of main/model.py:367-368 (common/nets/resnet.py, common/nets/module.py) under model.eval().
 * Forward only, exact f32, running statistics only (no training-mode BatchNorm, no backward).  Together with the whole-model
 * entries above: image + camera inputs in, joints / MANO mesh / object pose out, from a host with neither Python nor PyTorch.
 *   tensor table: every floating-point entry of backbone_net.* / decoder_net.* in state_dict() order (no num_batches_tracked), by
 *            checkpoint key, e.g. "backbone_net.resnet.layer1.0.conv1.weight"; a host maps a checkpoint by name.
 *   once   : hoisdf_encoder_prepared_bytes -> allocate -> hoisdf_encoder_prepare(tensors in table order): folds every BatchNorm
 *            (eps = 1e-5) into its convolution on the device and packs every weight.  The blob is self-contained.
 *   frame  : hoisdf_encoder_infer only enqueues on `stream`: img_nhwc [B][img_h][img_w][3] -> the five dense NHWC level buffers
 *            described by hoisdf_encoder_pyramid_shape (cfg.mutliscale_layers order: stride 2 .. 32; fill their pointers into the
 *            shape and hoisdf_pose_infer takes it as it is) and, when aux_out != NULL, [B][img_h / 2][img_w / 2][3] = heat-map (raw),
 *            hand and object segmentation (sigmoid).  prepared / workspace: 256-byte aligned device memory.
 * Refused with HOISDF_ERR_INVALID: an unknown depth, big_decoder below ResNet-50, image sides that are not multiples of 32, null
 * pointers, a short blob or workspace, n_tensors that is not the table's. */
typedef struct hoisdf_encoder_desc {
  int B, img_h, img_w;
  int resnet_type;                 /* 18 | 34 | 50 | 101 | 152 */
  int big_decoder;                 /* cfg.use_big_decoder (setting "ho3d"): 3968-channel pyramid, ResNet-50 and deeper */
} hoisdf_encoder_desc;
int hoisdf_encoder_tensor_count(const hoisdf_encoder_desc* desc);
const char* hoisdf_encoder_tensor_name(const hoisdf_encoder_desc* desc, int i);
long hoisdf_encoder_tensor_numel(const hoisdf_encoder_desc* desc, int i);
long hoisdf_encoder_prepared_bytes(const hoisdf_encoder_desc* desc);
int hoisdf_encoder_prepare(const hoisdf_encoder_desc* desc, const float* const* tensors, int n_tensors, void* prepared,
                           long prepared_bytes, void* stream);
long hoisdf_encoder_infer_workspace(const hoisdf_encoder_desc* desc);
int hoisdf_encoder_launch_count(const hoisdf_encoder_desc* desc);      /* kernels one hoisdf_encoder_infer (with aux_out) enqueues */
int hoisdf_encoder_pyramid_shape(const hoisdf_encoder_desc* desc, hoisdf_pyramid* shape_only);
int hoisdf_encoder_infer(const hoisdf_encoder_desc* desc, const void* prepared, const float* img_nhwc, float* const* level_out,
                         float* aux_out, void* workspace, long workspace_bytes, void* stream);

/* ---- (f4) auxiliary image losses of the encoder outputs ---------------------------------------------------
 * reference: main/model.py:128-143 (render_gaussian_heatmap) and :404-422 (MSELoss / BCELoss with reduction none).
 * dec = decoder_out (B, 3, H, W) [heat-map, hand seg, object seg] with element strides (sb, sc, sh, sw) - NCHW or
 * channels_last; joints (B, J, 2) = (x, y) in heat-map pixels; segs (B, H, W) in [0, 1].
 * heatmap (B, H, W) = 255 * sum_j exp(-((x - jx)/sigma)^2/2 - ((y - jy)/sigma)^2/2) (kept for the backward);
 * loss_heatmap = (dec0 - heatmap)^2, loss_*_seg = binary cross entropy with the log terms clamped at -100.
 * bwd: ddec gets all three channels (same strides as dec); a NULL upstream gradient means zero. */
int hoisdf_aux_image_losses_fwd(const float* dec, long sb, long sc, long sh, long sw, const float* joints,
                                const float* hand_seg, const float* obj_seg, int B, int J, int H, int W, float sigma,
                                float* heatmap, float* loss_heatmap, float* loss_obj_seg, float* loss_hand_seg,
                                void* stream);
int hoisdf_aux_image_losses_bwd(const float* dec, long sb, long sc, long sh, long sw, const float* hand_seg,
                                const float* obj_seg, const float* heatmap, const float* g_heatmap,
                                const float* g_obj_seg, const float* g_hand_seg, int B, int H, int W, float* ddec,
                                void* stream);

/* ---- (f4) BatchNorm2d (+ residual add) (+ ReLU) of a channels_last encoder map -------------------------------------
 * reference: the BatchNorm2d -> ReLU pairs and the `out += identity; relu(out)` block tails of common/nets/resnet.py (the
 * torchvision ResNet blocks it wraps) and common/nets/layer.py:23-63 (Conv / ConvTranspose -> BatchNorm2d -> ReLU), i.e.
 * torch.nn.functional.batch_norm(training) [+ add] + relu and its autograd backward.  The convolutions stay MIOpen's.
 * A channels_last (N, C, H, W) map is the row-major matrix [M = N H W][C] (row stride ld >= C, ld % 4 == 0; C % 8 == 0,
 * C <= 2048).  hoisdf_bn_stats: batch mean and 1 / sqrt(biased variance + eps) per channel (shifted f32 sums per block, f64
 * combination in slice order by a finishing kernel the same call queues: bit-reproducible), running statistics updated as
 * torch does (unbiased variance, momentum - a number: torch's momentum=None cumulative average is not offered; NULL = not tracked).  hoisdf_bn_apply_fwd: y [M][C] dense = relu?((x - mean) gamma invstd + beta
 * (+ residual)); second_is_variance = 1: the fourth argument holds variances (evaluation mode: the running statistics);
 * sign_bits [M][C / 8] bytes (bit j of byte (row, c / 8) = y[row][c + j] > 0; NULL = not wanted).  hoisdf_bn_bwd: dx [M][C]
 * dense, d_residual (NULL = no residual) = dy masked by the sign bits, dgamma / dbeta [C] overwritten (NULL = not wanted),
 * gamma NULL = no affine.  A NULL sign_bits MEANS that the forward applied no ReLU: the gradient then passes unmasked, so the
 * backward of a ReLU forward must hand in the map that forward wrote (there is no way to recompute it here).
 * workspace: hoisdf_bn_workspace_floats(M, C) floats. */
long hoisdf_bn_workspace_floats(long M, int C);
int hoisdf_bn_stats(const float* x, long ldx, long M, int C, float* mean, float* invstd, float* running_mean,
                    float* running_var, float momentum, float eps, float* workspace, long workspace_floats,
                    void* stream);
int hoisdf_bn_apply_fwd(const float* x, long ldx, const float* residual, long ldr, const float* mean,
                        const float* invstd_or_var, int second_is_variance, float eps, const float* gamma,
                        const float* beta, int relu, float* y, uint8_t* sign_bits, long M, int C, void* stream);
int hoisdf_bn_bwd(const float* dy, long lddy, const float* x, long ldx, const uint8_t* sign_bits, const float* mean,
                  const float* invstd, const float* gamma, float* dx, float* d_residual, float* dgamma, float* dbeta,
                  long M, int C, float* workspace, long workspace_floats, void* stream);

/* ---- optimizer step of the training loop ------------------------------------------------------------------
 * reference: torch.optim.AdamW(model.parameters(), lr=cfg.lr) (common/base.py:64-73; betas (0.9, 0.999), eps 1e-8,
 * weight_decay 1e-2 = torch defaults), stepped once per iteration (main/train.py:139).
 * chunks: device array; chunk i updates n <= 16384 consecutive elements of one parameter in place
 * (param, exp_avg, exp_avg_sq) from grad * grad_scale; step = 1-based count of this update (bias correction).
 * grad_scale = 1/world_size folds the gradient averaging of the all-reduce into the same pass.  Hyper-parameters are
 * doubles: 1 - beta2 formed from a float 0.999 is already 1.3e-5 off. */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
} hoisdf_adamw_chunk;
int hoisdf_adamw_step(const hoisdf_adamw_chunk* chunks, int n_chunks, double lr, double beta1, double beta2,
                      double eps, double weight_decay, long step, float grad_scale, void* stream);

/* ---- evaluation metrics: what main/test.py writes into results.txt, from device predictions ------------------------------
 * reference: common/metrics.py:62-232 (object and hand-joint metrics, the similarity alignment), common/eval_util.py:11-136
 * (EvalUtil.feed / get_measures, the F-score) as main/test.py:65-261 applies them.  csrc/eval.hip.  fp32 coordinates in metres
 * in; distances are dx^2 + dy^2 + dz^2 directly; no float atomics and one fixed order per sum: two calls give the same bits.
 * Every entry checks its arguments before any launch (HOISDF_ERR_INVALID names the argument); B = 0 returns 0, nothing launched.
 * hoisdf_eval_workspace_bytes(B, V): bytes of `workspace` that any entry below needs for B samples of V vertices (pure host
 *   arithmetic, -1 on B < 0 or V <= 0).  hoisdf_eval_accum_state_bytes(V, steps): bytes of an accumulator state (-1 on V <= 0
 *   or steps outside 2 .. 65535, the range every accumulator entry accepts).
 * hoisdf_eval_object (2 launches): obj_rot / obj_trans [B][P][3] = the P per-point predictions of a sample (axis-angle,
 *   translation), averaged over P; obj_rot_gt / obj_trans_gt [B][3]; both rotations through the quaternion Rodrigues form with
 *   the reference's + 1e-8; templates [T][V][3], obj_ids [B] int32 = the template of each sample.  Per sample, all four always:
 *   adds = mean over PREDICTED vertices of the distance to the nearest target vertex, mce = mean distance of the 8 axis-aligned
 *   bounding-box corners (corner order of common/metrics.py:70-72), oce = |trans - trans_gt|, mme = mean distance of
 *   corresponding vertices; used [B] = 1.  A sample with obj_ids[b] < 0 (HO3D's 019_pitcher_base rule, metrics.py:131-143) or
 *   >= T is not evaluated: its four outputs are 0 and used = 0.
 * hoisdf_eval_hand_joints (1 launch): pred / gt [B][J][3]; mje [B] = mean distance of corresponding points, pamje [B] = the same
 *   after the similarity (scale, rotation, translation) alignment of pred onto gt: fp64 centroids, H = (A-ca)^T (B-cb) / n and
 *   varP from the fp32 inputs, a Jacobi SVD of H with descending singular values, the reflection rule of metrics.py:195-198
 *   (det(V U^T) < 0: last singular value and last row of V^T negated), c = sum(s) / varP, t = cb - c R ca.  aligned_out
 *   [B][J][3] (may be NULL) = the aligned points rounded to fp32; transform_out [B][13] doubles (may be NULL) = c, R row-major,
 *   t; dist_out / dist_aligned_out [B][J] (each may be NULL) = the per-point distances before / after the alignment.  A rank-deficient H (collinear or coplanar points) takes one of the equally good rotations; pred points that are all
 *   equal (varP = 0) get c = 0.
 * hoisdf_eval_mesh (3 launches): pred / gt [B][V][3] meshes with corresponding vertices, thresholds [n_thresh] DEVICE doubles
 *   (1 <= n_thresh <= 16).  dist_raw / dist_aligned [B][V] = per-vertex distances before / after the alignment above (what the
 *   accumulator is fed); fscore / fscore_aligned [B][n_thresh] = eval_util.py:117-136 on brute-force nearest neighbours
 *   (precision = share of gt vertices with a pred vertex nearer than th, recall = the other way round, 2pr / (p + r), 0 when
 *   p + r = 0; fp32 distance compared in fp64, integer counts); aligned_out [B][V][3] may be NULL.
 * hoisdf_eval_accum_init / _feed / _finish: EvalUtil for fully visible meshes.  state = hoisdf_eval_accum_state_bytes(V, steps)
 *   device bytes, zeroed by _init: the number of samples fed, one fp64 sum per vertex, one uint32 count per (threshold,
 *   vertex) of d <= th (fp32 distance compared in fp64).  thresholds [steps] DEVICE doubles, the same array for every feed and
 *   the finish.  _feed adds dist [B][V]; one thread owns a vertex and walks the samples in order, so feeding 3 + 3 samples
 *   and feeding 6 leave the same bits.  _finish writes out [2 + steps] DEVICE doubles: the mean EPE, the AUC (trapezoid of the
 *   per-threshold PCK over the thresholds, normalised by their range, mean over vertices) and the PCK curve; NaN before the
 *   first feed.  The median EPE of get_measures is not provided (it needs every distance; results.txt does not print it). */
long hoisdf_eval_workspace_bytes(int B, int V);
long hoisdf_eval_accum_state_bytes(int V, int steps);
int hoisdf_eval_object(const float* obj_rot, const float* obj_trans, int P, const float* obj_rot_gt, const float* obj_trans_gt,
                       const float* templates, int T, int V, const int32_t* obj_ids, int B, float* adds, float* mce, float* oce,
                       float* mme, int32_t* used, void* workspace, long workspace_bytes, void* stream);
int hoisdf_eval_hand_joints(const float* pred, const float* gt, int B, int J, float* mje, float* pamje, float* aligned_out,
                            double* transform_out, float* dist_out, float* dist_aligned_out, void* stream);
int hoisdf_eval_mesh(const float* pred, const float* gt, int B, int V, const double* thresholds, int n_thresh, float* dist_raw,
                     float* dist_aligned, float* fscore, float* fscore_aligned, float* aligned_out, void* workspace,
                     long workspace_bytes, void* stream);
int hoisdf_eval_accum_init(void* state, int V, int steps, void* stream);
int hoisdf_eval_accum_feed(void* state, const float* dist, int B, int V, const double* thresholds, int steps, void* stream);
int hoisdf_eval_accum_finish(const void* state, int V, const double* thresholds, int steps, double* out, void* stream);

/* ---- image preparation: from a camera frame to the model input --------------------------------------------------------------
 * reference: the image half of Dataset.__getitem__ (data/dexycb.py:219-404 data_aug / data_crop, data/ho3d.py:399-427 data_crop,
 * data/dataset_util.py get_bbox_joints, fuse_bbox, get_affine_transform, transform_coords, transform_img, color_jitter).
 * csrc/imgprep_params.c (host arithmetic, no GPU call) and csrc/imgprep.hip (kernels); hoisdf_amd/image_oracle.py restates both.
 *
 * hoisdf_crop_params_dexycb / _ho3d / hoisdf_aug_params_dexycb fill a hoisdf_crop on the host.  Number formats are the
 *   reference's: boxes of float32 joints and the evaluation affine are float32 arithmetic, the rest float64; affine,
 *   post_rot_trans and rot_mat are the float32 matrices get_affine_transform returns; `inverse` = the first two rows of the
 *   float64 inverse of that float32 affine.  joints_uv [n_joints][2] float32 and p2d [n_corners][2] float64 are the labels of the
 *   RAW frame (at most HOISDF_CROP_MAX_POINTS each); K [9] row-major; flip != 0 (a left hand) mirrors them first
 *   (u -> W - u - 1, K[0][2] -> W - K[0][2] - 1) and the warp then reads the raw frame mirrored.  res = input_img_shape[0],
 *   hm = output_hm_shape[0].  Out: K = K' (dexycb: post_rot_trans . K, ho3d: affine . K), bbox_hand / bbox_obj in crop pixels,
 *   joints_uv at heat-map scale, p2d normalised to bbox_obj.  The training variant takes the random numbers as arguments:
 *   centre offset = center_jittering * scale * center_u[0..1], scale *= scale_jitter, rotation `rot` in radians.
 *   HOISDF_ERR_INVALID: null pointer, point counts outside 1 .. HOISDF_CROP_MAX_POINTS, res / hm / frame size <= 0, a
 *   degenerate (empty or non-finite) fused box.
 * hoisdf_image_crop (evaluation, 1 launch per 16 samples): frames[b] describes sample b's DEVICE buffers: frame u8 [H][W][3],
 *   hand_mask / obj_mask u8 [H][W] bytes or, mask_packed != 0, bits as numpy.packbits leaves them (bit 7 of byte 0 first).
 *   crops [B] is HOST memory (inverse and flip are read).  Output pixel (x, y) takes source pixel
 *   (floor(t00 (x + .5) + t01 (y + .5) + t02), floor(t10 (x + .5) + t11 (y + .5) + t12)) evaluated in float64 without fused
 *   multiply-add, 0 outside the frame (PIL's Image.AFFINE with its default nearest filter).  img = level / 255 as float32,
 *   [B][res][res][3] (nchw = 0, what hoisdf_encoder_infer consumes) or [B][3][res][res]; crop_u8 [B][res][res][3] may be NULL;
 *   hand_seg / obj_seg [B][hm][hm] float32: heat-map pixel i reads crop pixel floor((i + .5) res / hm) of the same map (the
 *   NEAREST resize folded in, no res x res mask is written).
 * hoisdf_image_augment (training): the same warp into crop_u8 (required), then per sample photo[b] (HOST memory): a separable
 *   7-tap Gaussian blur of sigma blur_sigma (edges replicated, rounded to the nearest level, the identity below 0.05), then the
 *   enabled ones of brightness (0), contrast (1), saturation (2), hue (3) in the order `order` gives, each leaving integer levels
 *   0 .. 255: out = trunc(clip(deg + f (x - deg), 0, 255)) in float32 with deg = 0, int(mean(L) + .5) over the crop, L per pixel;
 *   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; hue = PIL's RGB -> HSV, H += uint8(factor 255) modulo 256, HSV -> RGB.
 *   lsum [B] uint32 DEVICE: the integer sum of L the contrast of sample b saw (integer atomics: order-independent; 0 when contrast
 *   is off).  Launches per 16 samples: the warp; a memset of lsum; when any sample has a contrast, the chain up to it; the chain.
 * Both only enqueue on `stream`, check every argument before the first launch (HOISDF_ERR_INVALID: null pointer, res / hm <= 0,
 *   res % hm != 0, frame size <= 0, a singular or non-finite inverse, enabled bits outside 0 .. 15, an order that is no
 *   permutation of 0 .. 3, a negative or non-finite blur_sigma / factor) and return 0 for B = 0. */
#define HOISDF_CROP_MAX_POINTS 32
typedef struct {
  float affine[9];
  float post_rot_trans[9];
  float rot_mat[9];
  double inverse[6];
  double K[9];
  double bbox_hand[4];
  double bbox_obj[4];
  int n_joints, n_corners, flip, reserved;
  double joints_uv[HOISDF_CROP_MAX_POINTS][2];
  double p2d[HOISDF_CROP_MAX_POINTS][2];
} hoisdf_crop;
typedef struct {
  const uint8_t* frame;
  const uint8_t* hand_mask;
  const uint8_t* obj_mask;
  int H, W;
  int mask_packed, reserved;
} hoisdf_frame;
typedef struct {
  float blur_sigma;
  float factor[4];
  int enabled;       /* bit i: op i is present */
  int order[4];
} hoisdf_photo;
int hoisdf_crop_params_dexycb(const float* joints_uv, int n_joints, const double* p2d, int n_corners, const double* K, int frame_w,
                              int frame_h, int flip, int res, int hm, hoisdf_crop* out);
int hoisdf_crop_params_ho3d(const double* bbox_hand, const double* p2d, int n_corners, const double* K, int frame_w, int frame_h,
                            int res, int hm, hoisdf_crop* out);
int hoisdf_aug_params_dexycb(const float* joints_uv, int n_joints, const double* p2d, int n_corners, const double* K, int frame_w,
                             int frame_h, int flip, int res, int hm, double center_jittering, const double* center_u,
                             double scale_jitter, double rot, hoisdf_crop* out);
int hoisdf_image_crop(const hoisdf_frame* frames, const hoisdf_crop* crops, int B, int res, int hm, int nchw, float* img,
                      uint8_t* crop_u8, float* hand_seg, float* obj_seg, void* stream);
int hoisdf_image_augment(const hoisdf_frame* frames, const hoisdf_crop* crops, const hoisdf_photo* photo, int B, int res, int hm,
                         int nchw, float* img, uint8_t* crop_u8, uint32_t* lsum, float* hand_seg, float* obj_seg, void* stream);

/* ---- mesh SDF: the rows [x y z sdf_hand sdf_obj label] of sdf_processed/<frame>.npy from the two meshes of a step ------------
 * reference: tool/pre_process_sdf.py:140-148 only REPACKS such rows; the mesh-to-SDF pass that makes them is an offline CPU tool
 * outside the reference.  csrc/mesh_sdf.hip; hoisdf_amd/mesh_sdf_oracle.py restates it in numpy.  Lengths are metres in the frame
 * of the vertices (camera metres for the training path); no gradient; fixed order everywhere: two calls give the same bits.
 * Every entry checks its arguments before any launch (HOISDF_ERR_INVALID: a required pointer null, a negative count, B > 65535,
 *   max_faces > HOISDF_MESH_MAX_FACES, a row stride too short) and returns 0 with nothing launched for B = 0 or N = 0.
 *
 * hoisdf_mesh_prepare (1 launch): verts [B][V][3]; faces int32 [max_faces][3] shared by the batch (face_batch_stride = 0) or
 *   [B][...] with face_batch_stride int32 elements (>= 3 max_faces) between samples; n_faces [B] DEVICE int32 (NULL: max_faces
 *   everywhere; values are clamped to 0 .. max_faces): face rows from n_faces[b] on are padding and are never read.  Faces are
 *   wound counter-clockwise seen from outside.  Out, per sample: tris [B][max_faces][12] floats (16-byte aligned) = the three
 *   corners minus the sample's CENTRE, each followed by its vertex index as int32 bits (-1 in the first slot: a skipped face);
 *   area [B][max_faces]; cdf [B][max_faces] = the inclusive prefix sum of the areas in face order; box [B][8] = centre xyz, total
 *   area, half extent xyz, 0.  The centre is that of the bounding box of the sample's V vertices: the queries subtract it too, so
 *   the fp32 arithmetic happens at the size of the mesh, not at its camera depth.
 *   Skipped-face rule: a face whose normal (b - a) x (c - a), every product rounded on its own, is exactly (0, 0, 0) - two equal
 *   indices, coincident points - or which names a vertex outside 0 .. V-1 is skipped: area 0 (the sampler never picks it), no
 *   part in distance or sign.
 * hoisdf_mesh_sample_points (1 launch): N points per sample into points[(b N + i) ldp + 0..2] (ldp >= 3), stateless: a pure
 *   function of (seed, b, i).  Kind of point i, from i alone: with k = i mod uniform_every, k = uniform_every - 1 is UNIFORM in
 *   the box (half extent + pad); otherwise near-surface with sigma1 (k even) or sigma2 (k odd); uniform_every <= 0: no uniform
 *   points, k = i.  Near-surface: face = the first with cdf > u total (area-weighted), barycentrics (1 - sqrt(u1),
 *   sqrt(u1) (1 - u2), sqrt(u1) u2), plus isotropic Gaussian noise of that sigma.  A mesh without area gets box points only.
 *   face_out [B][N] int32 (may be NULL) = the face picked, -1 for a box point.
 * hoisdf_mesh_sdf (1 launch): points[(b N + i) ldp + 0..2] against the prepared mesh of sample b.  For every face not skipped:
 *   the exact closest point of the triangle (vertex, edge and face regions) and the solid angle 2 atan2(det[a b c], |a||b||c| +
 *   (a.b)|c| + (b.c)|a| + (c.a)|b|) of the corners seen from the point.
 *   Sign rule: winding = sum of the solid angles / 4 pi; sdf = -distance where winding > 0.5, else +distance.  (Not
 *   pseudonormals: the hand mesh is open at the wrist and templates need not be manifold; the winding number degrades
 *   gracefully on both.)  Tie rule: faces are visited in ascending order and a face replaces the best only when strictly
 *   nearer, so the LOWEST face index wins an exact tie; likewise the earliest corner wins equal barycentric weights.
 *   sdf[(b N + i) ld] (ld >= 1: pass the address of the column - outputs land in a column of a wider row block); optional,
 *   may be NULL: face_out [B][N] int32 (-1: no usable face; the distance is then 3e38), bary_out [B][N][3] = weights of the
 *   face's corners at the closest point, winding_out [B][N], label_out [B][N] int32 = vert_label[the corner with the largest
 *   weight] (vert_label int32 [V], label_batch_stride elements between samples, 0 = shared; required with label_out).
 * hoisdf_mesh_sdf_rows (6 launches): the composite.  rows [B][n_hand + n_obj][ld] floats, ld >= 6, in the layout of
 *   tool/pre_process_sdf.py:140-148: per sample n_hand points sampled at the hand mesh, then n_obj sampled at the object mesh
 *   (seeds 2 seed and 2 seed + 1); on EVERY row column 3 = sdf to the hand, column 4 = sdf to the object; column 5 = the hand
 *   part hand_vert_label[..] where the row is a hand row and |sdf_hand| <= clamp, else -1 (object rows: always -1); columns from
 *   6 on are not touched.  The reference applies its clamp in units normalised by its hand scale; here clamp is metres and a
 *   parameter.  workspace: hoisdf_mesh_sdf_rows_workspace_bytes(B, hand max_faces, obj max_faces) device bytes (-1 on an
 *   invalid shape), 256-byte aligned. */
#define HOISDF_MESH_MAX_FACES 4096
#define HOISDF_MESH_TILE 128
typedef struct {
  const float* verts;
  const int32_t* faces;
  const int32_t* n_faces;
  long face_batch_stride;
  int V, max_faces;
} hoisdf_mesh;
int hoisdf_mesh_prepare(const float* verts, int B, int V, const int32_t* faces, long face_batch_stride, const int32_t* n_faces,
                        int max_faces, float* tris, float* area, float* cdf, float* box, void* stream);
int hoisdf_mesh_sample_points(const float* tris, const float* cdf, const float* box, const int32_t* n_faces, int max_faces, int B,
                              int N, float sigma1, float sigma2, int uniform_every, float pad, uint64_t seed, float* points,
                              int ldp, int32_t* face_out, void* stream);
int hoisdf_mesh_sdf(const float* points, int ldp, int B, int N, const float* tris, const float* box, const int32_t* n_faces,
                    int max_faces, const int32_t* vert_label, long label_batch_stride, float* sdf, int ld, int32_t* face_out,
                    float* bary_out, float* winding_out, int32_t* label_out, void* stream);
long hoisdf_mesh_sdf_rows_workspace_bytes(int B, int hand_max_faces, int obj_max_faces);
int hoisdf_mesh_sdf_rows(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* hand_vert_label, int B, int n_hand,
                         int n_obj, float sigma1, float sigma2, int uniform_every, float pad, float clamp, uint64_t seed,
                         float* rows, int ld, void* workspace, long workspace_bytes, void* stream);

/* ---- interaction: penetration depth, contact and intersection volume of a posed hand mesh and a posed object mesh ---------------
 * reference: none - the reference evaluates every prediction against ground truth and never the hand against the object.  These
 * are the three numbers hand-object work reports since ObMan (Hasson et al., CVPR 2019), at ObMan's 5 mm voxels.
 * csrc/interact.hip; hoisdf_amd/interaction_oracle.py restates it in numpy.  Both meshes as hoisdf_mesh_sdf_rows takes them, in ONE
 * frame, lengths in metres (volume: cubic metres); no gradient; fixed order everywhere: two calls give the same bits.
 * hoisdf_eval_interaction (6 launches: hoisdf_mesh_prepare x 2, hoisdf_mesh_sdf x 2, the voxel pass, the per-sample reduction).
 *   Checked before the first launch (HOISDF_ERR_INVALID, the argument named in hoisdf_last_error): hand, obj, verts, faces, a
 *   required output or the workspace null; B < 0 or B > 65535; a mesh without vertices; max_faces > HOISDF_MESH_MAX_FACES; a
 *   face_batch_stride that is neither 0 nor >= 3 max_faces; contact_dist < 0 or not finite; voxel <= 0 or not finite; a workspace
 *   below hoisdf_eval_interaction_workspace_bytes(B, hand V, hand max_faces, obj V, obj max_faces) device bytes (-1 on an invalid
 *   shape; 256-byte aligned).  B = 0 returns 0 with nothing launched.  It only enqueues on `stream`.
 *   Vertex pass: sdf_obj(v) of every hand vertex to the object mesh and sdf_hand(v) of every object vertex to the hand mesh, by
 *   hoisdf_mesh_sdf: its distance, its tie rule and its sign rule (winding > 0.5 is inside, so the hand's open wrist is handled;
 *   a mesh without a usable face is 3e38 away).  obj_n_verts [B] DEVICE int32 (NULL: obj->V everywhere; clamped to 0 .. obj->V):
 *   object vertex rows from obj_n_verts[b] on are padding and take no part in pen_obj.  They DO take part in the object's
 *   bounding box, as every row of a hoisdf_mesh does: pad with copies of a real vertex.  Per sample, all [B]:
 *     pen_hand       max over the hand vertices of max(0, -sdf_obj)
 *     pen_obj        max over the sample's object vertices of max(0, -sdf_hand)
 *     min_dist       min over the hand vertices of |sdf_obj|
 *     contact_verts  int32: the number of hand vertices with sdf_obj <= contact_dist (a vertex inside the object counts)
 *     in_contact     int32: 1 if contact_verts > 0 or pen_obj > 0, else 0
 *   An object without a usable face: pen_hand = pen_obj = 0, contact_verts = in_contact = 0, min_dist = 3e38.
 *   Voxel pass.  Grid rule, per sample and per axis, in fp32 and in this order, no product fused into a sum, from the two box[8]
 *   of hoisdf_mesh_prepare (c = centre, h = half extent):  lo = max(c_hand - h_hand, c_obj - h_obj);  hi = min(c_hand + h_hand,
 *   c_obj + h_obj);  extent = hi - lo;  n = min(ceil(extent / voxel), HOISDF_INTERACT_MAX_GRID), at least 1;  cell = extent / n:
 *   the cells tile the overlap of the two bounding boxes exactly.  Any extent <= 0: n = 0 on every axis, no cell, volume 0.
 *   Cell i = ix + n_x (iy + n_y iz) (ix fastest) has the centre lo + (ix + 0.5) cell (product, then sum).  For each centre only the
 *   winding number against each mesh is taken (hoisdf_mesh_sdf's solid angles, its skipped-face rule, tiles of HOISDF_MESH_TILE
 *   faces and a fixed summation order per centre); a cell is inside when winding_obj > 0.5 and winding_hand > 0.5.  The object comes
 *   first, and a workgroup of 64 cells none of which is inside the object skips the hand.
 *     inside_count   int32 [B]: the number of inside cells (integer sums: independent of any order)
 *     volume         [B]: ((inside_count cell_x) cell_y) cell_z in fp32, cubic metres
 *     inside_out     uint8 [B][HOISDF_INTERACT_MAX_GRID^3], may be NULL: 1 / 0 per cell i; bytes from n_x n_y n_z on are not touched
 *     grid_out       [B][8] floats, may be NULL: lo xyz, cell xyz, n_x | n_y << 8 | n_z << 16 as int32 bits, 0 */
#define HOISDF_INTERACT_MAX_GRID 64
long hoisdf_eval_interaction_workspace_bytes(int B, int hand_V, int hand_max_faces, int obj_V, int obj_max_faces);
int hoisdf_eval_interaction(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, int B,
                            float contact_dist, float voxel,
                            float* pen_hand, float* pen_obj, float* min_dist, int32_t* contact_verts, int32_t* in_contact,
                            float* volume, int32_t* inside_count, uint8_t* inside_out, float* grid_out,
                            void* workspace, long workspace_bytes, void* stream);

/* ---- interaction loss: the same quantities in a form to train against - repulsion and attraction, with their gradients ------------
 * reference: none - the reference trains every part against ground truth and never couples the hand to the object.  ObMan (Hasson
 * et al., CVPR 2019) trains with a repulsion of the vertices that lie inside the other mesh and a saturating attraction of contact
 * zones onto the surface; these are those two terms on hoisdf_mesh_sdf's exact distance.  csrc/interact_loss.hip;
 * hoisdf_amd/interaction_loss_oracle.py restates it in numpy.  Both meshes as hoisdf_eval_interaction takes them, in ONE frame,
 * lengths in metres; obj_n_verts as there (padding object vertices take no part and, as query points, get no gradient).  A mesh whose
 * face count is 0 is absent: its vertices are no query points either, so such a sample gives three zeros and zero gradients.
 * Weights, each may be NULL = all ones: rep_w_hand, att_w_hand [hand V] and rep_w_obj [obj V] floats per sample, with a batch stride
 *   in elements of 0 (one array shared by the batch) or V.  alpha > 0: the length at which the attraction saturates.
 * Checked before the first launch by both entries (HOISDF_ERR_INVALID, the argument named in hoisdf_last_error): hand, obj, verts,
 *   faces, an output or the workspace null; B < 0 or B > 65535; a mesh without vertices; max_faces > HOISDF_MESH_MAX_FACES; a
 *   face_batch_stride that is neither 0 nor >= 3 max_faces; a weight stride that is neither 0 nor V; alpha <= 0 or not finite; a
 *   workspace below hoisdf_interaction_loss_workspace_bytes(B, hand V, hand max_faces, obj V, obj max_faces) device bytes (-1 on an
 *   invalid shape; 256-byte aligned).  B = 0 returns 0 with nothing launched.  Both only enqueue on `stream`.
 * hoisdf_interaction_loss_fwd (5 launches: hoisdf_mesh_prepare x 2, hoisdf_mesh_sdf x 2, the per-sample reduction).  With sdf_obj(v)
 *   of hand vertex v to the object mesh and sdf_hand(v) of object vertex v to the hand mesh - hoisdf_mesh_sdf's distance, tie rule
 *   and sign rule - per sample, all [B]:
 *     rep_hand = sum_v rep_w_hand[v] max(0, -sdf_obj(v)) / sum_v rep_w_hand[v]                      over the hand vertices
 *     att      = sum_v att_w_hand[v] alpha tanh(max(0, sdf_obj(v)) / alpha) / sum_v att_w_hand[v]   over the hand vertices
 *     rep_obj  = sum_v rep_w_obj[v] max(0, -sdf_hand(v)) / sum_v rep_w_obj[v]                       over v < obj_n_verts[b]
 *   The denominators do not depend on the geometry; one that is not positive gives 0.  A query point whose mesh has no usable face
 *   (distance 3e38) adds 0 to every numerator.  Sums in fp64: thread t of 256 takes vertices t, t + 256, ... in ascending order, the
 *   256 partial sums meet in the fixed tree s[t] += s[t + 128], s[t + 64], ... ; one rounding to fp32.
 *   The workspace keeps sdf, winning face and barycentric weights of every query point of both directions, the prepared meshes and
 *   the denominators: hoisdf_interaction_loss_bwd reads them, so between the two calls the workspace, both vertex arrays, the
 *   faces, the counts, the weights and alpha stay as they were.
 * hoisdf_interaction_loss_bwd (2 launches, one per destination mesh): upstream gradients g_rep_hand, g_att, g_rep_obj [B] (any may
 *   be NULL = zero) -> d_hand_verts [B][hand V][3], d_obj_verts [B][obj V][3]; every row is written, a padding row gets 0.
 *   Rule: with c = sum_k beta_k x_k the closest point on the winning face of query point p, d = |p - c|, n = (p - c) / d and the sign
 *   s held piecewise constant, d sdf / d p = s n and d sdf / d x_k = -beta_k s n (the envelope rule: face, edge and corner regions
 *   alike).  coef(p) = the derivative of p's terms by sdf - -1 for the repulsion where sdf < 0, 1 - tanh^2(sdf / alpha) for the
 *   attraction where sdf > 0 - times the weight, divided by the denominator, times the upstream gradient.  A vertex receives
 *   (1) its own term coef s n as a query point and (2) -beta_k coef s n of every query point of the OTHER mesh whose winning face
 *   names it as corner k.  A point with d = 0, without a usable face or past obj_n_verts contributes nothing.
 *   Order: no atomics; each destination vertex is owned by one lane, which adds in fp64 its own term first, then the other mesh's
 *   query points in ASCENDING query index (staged through LDS in tiles of HOISDF_INTERACT_LOSS_TILE records), corners 0, 1, 2 within
 *   a record, and rounds to fp32 once.  Two calls give the same bits; a batch equals its samples run one by one, bit for bit. */
#define HOISDF_INTERACT_LOSS_TILE 64
long hoisdf_interaction_loss_workspace_bytes(int B, int hand_V, int hand_max_faces, int obj_V, int obj_max_faces);
int hoisdf_interaction_loss_fwd(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, int B,
                                const float* rep_w_hand, long rep_w_hand_stride, const float* att_w_hand, long att_w_hand_stride,
                                const float* rep_w_obj, long rep_w_obj_stride, float alpha,
                                float* rep_hand, float* att, float* rep_obj, void* workspace, long workspace_bytes, void* stream);
int hoisdf_interaction_loss_bwd(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, int B,
                                const float* rep_w_hand, long rep_w_hand_stride, const float* att_w_hand, long att_w_hand_stride,
                                const float* rep_w_obj, long rep_w_obj_stride, float alpha,
                                const float* g_rep_hand, const float* g_att, const float* g_rep_obj,
                                float* d_hand_verts, float* d_obj_verts, const void* workspace, long workspace_bytes, void* stream);

/* ---- iso-surface: a sampled field as an indexed triangle mesh, and its Chamfer distance to a ground-truth mesh -------------------
 * reference: none - the reference reads its two fields only at the points sdf_infer ranks.  AlignSDF and gSDF, which its field
 * code descends from, report the Chamfer distance of the extracted zero level set.  csrc/isosurf.hip;
 * hoisdf_amd/isosurf_oracle.py restates the rules below in numpy.  No gradient.  Every slot is decided by integer prefix sums
 * over a fixed element order and every floating-point sum has one order: two calls give the same bits.
 * Every entry checks its arguments before any launch (HOISDF_ERR_INVALID, the argument named in hoisdf_last_error: a required
 *   pointer null, B < 0 or B > 65535, n < 2 or n > HOISDF_ISO_MAX_GRID, ld < 1, a negative capacity, a workspace below the size
 *   query, which itself returns -1 on an invalid shape), returns 0 with nothing launched for B = 0, and only enqueues on `stream`.
 *
 * Grid: per sample grid [B][8] floats = lo xyz, cell xyz, 0, 0; the batch shares n nodes per axis.  Node i = ix + n (iy + n iz)
 *   (ix fastest) sits at lo + ix cell per axis, in fp32, the product rounded before the sum.  Coordinates are in the frame of
 *   the caller's field (for the model: the scaled frame of sdf_infer's lattice).
 * hoisdf_iso_grid_points (1 launch): points [B n^3][3] = the node positions, sample_idx [B n^3] int32 (may be NULL) = b: the
 *   rows hoisdf_sdf_query_fwd takes.
 * hoisdf_iso_refine_grid (1 launch, no host read): values [B][n^3], element (b, i) at values[(b n^3 + i) ld].  Per sample and
 *   axis the smallest and largest index of a node with value < iso (integer min / max), grown by pad_cells (0 .. 128) and
 *   clipped to 0 .. n - 1 -> i0, i1;  lo_out = lo + i0 cell;  cell_out = ((lo + i1 cell) - lo_out) / (n_out - 1): the n_out
 *   nodes span that box exactly.  A sample without such a node: i0 = 0, i1 = n - 1 (the coarse grid re-divided).
 * hoisdf_iso_extract (2 launches to count, 4 with output): marching tetrahedra on the Kuhn subdivision.
 *   A node is INSIDE when value < iso (strict: a value equal to iso is outside).  A cell (its 000 corner p, ix, iy, iz < n - 1) is
 *   cut into six tetrahedra around its diagonal 000 -> 111: tetrahedron k has the corners p, p + e_a, p + e_a + e_b, p + 111 (in
 *   this order: corners 0..3) for the k-th permutation (a, b, c) of the axes in lexicographic order (xyz, xzy, yxz, yzx, zxy,
 *   zyx).  The subdivision is the same in every cell and matches across cell faces: the surface has no cracks.
 *   Vertices live on grid edges.  Node p owns the 7 edges p -> p + d, d = 100, 010, 001, 110, 101, 011, 111 (edges 0..6; every
 *   tetrahedron edge is one of these).  An owned edge is ACTIVE when the far node exists, both values are finite and exactly
 *   one end is inside.  Vertex order: ascending node index, then ascending edge number.  Position: a = the inside end, b = the
 *   outside end, t = (iso - v_a) / (v_b - v_a), per axis x = x_a + t (x_b - x_a) with x_a, x_b by the grid rule, the product
 *   rounded before the sum: one formula per vertex, whichever end owns it.  With out_shift [B][3] (NULL: skipped, out_scale
 *   ignored) the stored vertex is x out_scale + out_shift[b] (product, then sum): 1 / sdf_scale and the sample's centre give
 *   camera metres.
 *   Faces: ascending cell index (= the node index of its 000 corner), tetrahedron 0..5, then the case's triangles.  A cell with
 *   a corner that is not finite emits nothing.  With the inside corners of a tetrahedron i (< j (< k)) and the outside ones
 *   o (< p (< q)), edges named by their two corners: one inside corner -> the triangle (io, ip, iq); three -> (oi, oj, ok); two ->
 *   the quad io, ip, jp, jo cut along io - jp into (io, ip, jp) and (io, jp, jo); each triangle then reversed (its last two
 *   vertices swapped) where needed to be wound counter-clockwise seen from the outside (the value > iso side): hoisdf_mesh's
 *   convention.  Zero-area triangles (t = 1 at several edges of one node) are kept: hoisdf_mesh_prepare skips them.
 *   verts [B][max_verts][3], faces int32 [B][max_faces][3] (vertex ids within the sample), n_verts / n_faces [B] DEVICE int32 =
 *   the counts NEEDED, which may exceed the capacities: rows beyond a capacity are not written, written faces keep their true
 *   vertex ids, and the caller compares counts and capacities.  verts NULL or faces NULL: that output is skipped (its capacity
 *   is ignored); both NULL: the call only counts - read the counts back once, allocate exactly, call again.
 *   workspace: hoisdf_iso_extract_workspace_bytes(B, n) device bytes, 256-byte aligned.
 * hoisdf_eval_surface (5 launches: hoisdf_mesh_prepare, hoisdf_mesh_sdf, hoisdf_mesh_sample_points, nearest vertex, reduction):
 *   pred_verts [B][max_verts][3] with pred_n_verts [B] DEVICE int32 (clamped to 0 .. max_verts; rows beyond are read but take
 *   no part; max_verts <= 2^24) against the ground-truth mesh gt (as hoisdf_mesh_sdf_rows takes it), one frame, metres.
 *     pred_to_gt [B]  mean over the sample's predicted vertices of the SQUARED distance to the mesh (hoisdf_mesh_sdf: exact
 *                     point-to-triangle distance, its tie and skipped-face rules)
 *     gt_to_pred [B]  mean over n_samples (1 .. 2^24) points drawn on the mesh by area (hoisdf_mesh_sample_points with both
 *                     sigmas 0 and uniform_every 0: the barycentric point itself; a pure function of seed, b, i) of the squared
 *                     distance to the nearest predicted vertex (brute force; the lowest index wins an exact tie)
 *     chamfer [B]     their sum, square metres;   n_used [B] int32 = the vertex count that took part
 *   Both means are fp64 sums in a fixed order, stored as floats.  A sample without a predicted vertex, or whose mesh has no
 *   area (no usable face): n_used = 0 and zeros.  Optional, may be NULL: samples_out [B][n_samples][3] = the drawn points,
 *   nearest_out [B][n_samples] int32 = the nearest vertex (-1: none).
 *   workspace: hoisdf_eval_surface_workspace_bytes(B, max_verts, gt max_faces, n_samples) device bytes, 256-byte aligned. */
#define HOISDF_ISO_MAX_GRID 128
int hoisdf_iso_grid_points(const float* grid, int n, int B, float* points, int32_t* sample_idx, void* stream);
int hoisdf_iso_refine_grid(const float* values, int ld, const float* grid_in, int n, int B, float iso, int pad_cells, int n_out,
                           float* grid_out, void* stream);
long hoisdf_iso_extract_workspace_bytes(int B, int n);
int hoisdf_iso_extract(const float* values, int ld, const float* grid, int n, int B, float iso, float out_scale,
                       const float* out_shift, float* verts, int max_verts, int32_t* faces, int max_faces, int32_t* n_verts,
                       int32_t* n_faces, void* workspace, long workspace_bytes, void* stream);
long hoisdf_eval_surface_workspace_bytes(int B, int max_verts, int gt_max_faces, int n_samples);
int hoisdf_eval_surface(const float* pred_verts, const int32_t* pred_n_verts, int max_verts, const hoisdf_mesh* gt, int B,
                        int n_samples, uint64_t seed, float* pred_to_gt, float* gt_to_pred, float* chamfer, int32_t* n_used,
                        float* samples_out, int32_t* nearest_out, void* workspace, long workspace_bytes, void* stream);

/* ---- field fit: a point set moved, as a rigid body, onto the zero level set of a sampled signed-distance field ------------------
 * reference: none - the reference never feeds its fields back into the pose.  Grasping Field, AlignSDF and gSDF, which its field
 * code descends from, fit the predicted mesh to the predicted field at test time.  csrc/field_fit.hip (the launches and the
 * summation order) and csrc/field_fit_rules.h (the rules as plain functions, compiled for the host too);
 * hoisdf_amd/field_fit_oracle.py states the rules in full - order of every operation included - and restates them in numpy
 * float64.  A damped Gauss-Newton (Levenberg-Marquardt) fit per sample; rigid only; no gradient.  All arithmetic is fp64 on the
 * f32 inputs, every product and sum rounded on its own, every sum in one order: two calls give the same bits, and a sample of a
 * batch gets the bits it gets alone.
 *
 * hoisdf_field_fit (hoisdf_field_fit_launch_count(iters) = iters + 2 launches on `stream`, never synchronises):
 *   values [B][ld] floats, ld >= n^3: the field of sample b on its grid, node i = ix + n (iy + n iz) at values[b ld + i];
 *   grid [B][8] = lo xyz, cell xyz, 0, 0; n in 2 .. HOISDF_ISO_MAX_GRID: what hoisdf_iso_extract takes.  points [B][V][3] in the
 *   frame of the field (V <= 2^24); n_points [B] DEVICE int32 or NULL = V, clamped to 0 .. V: rows beyond are not read, and their
 *   rows of points_out are not written.  pivot [B][3] or NULL = the mean of the sample's points.
 *   Pose: x = R (p - c) + c + t from R = I, t = 0.  A point TAKES PART when it lies on the grid (0 <= u <= n - 1 per axis, a NaN
 *   fails) and the 8 corners of its cell are finite.  Cost: the mean over those points of the Huber function (threshold `huber` >
 *   0, field units) of the trilinear interpolant f.  Step: J = [g, r x g] with g the interpolant's analytic gradient and r the
 *   rotated offset (a left perturbation about c + t); (H + lambda diag(H) + 1e-12 I) d = -b by a 6 x 6 Cholesky factorisation, a
 *   pivot that is not > 0 counting as a rejected step; R' = exp(omega) R by Rodrigues, t' = t + delta.  ACCEPT when the trial has
 *   a point, 100 n_used >= min_used_percent x the start pose's n_used and the cost is strictly smaller: lambda <- max(lambda / 10,
 *   1e-9); otherwise lambda <- 10 lambda, and the sample stops once lambda > 1e9.  lambda starts at lambda0 (>= 0).  The stop
 *   test comes before a step is tried: after `iters` (0 .. HOISDF_FIELD_FIT_MAX_ITERS) tried steps, rejected ones included, or
 *   when the solved step is below step_tol (max of |delta| and |omega| x the largest |p - c|).  A stopped sample does not change.
 *   Launches: one workgroup of 256 lanes per sample.  init: pivot, extent, the sums of the start pose, the first plan (stop
 *   tests, solve, trial pose).  round x iters: the sums at the trial pose, accept / reject, the next plan; the workgroup of a
 *   stopped sample returns at once.  finish: the outputs.  The iteration is the host's fixed sequence of launches: no kernel has
 *   a barrier inside a loop.  Sums: lane l takes points l, l + 256, ... ascending, an xor tree over 32 .. 1 within each wave of
 *   64, then ((wave 0 + wave 1) + wave 2) + wave 3.
 *   Outputs: rot [B][9] (row-major), trans [B][3], points_out [B][V][3] = ((R (p - c) + c) + t) as floats, each rounded once from
 *   fp64; cost [B][2] doubles = the start pose's and the final cost; info [B][4] int32 = points that take part at the start, at
 *   the end, steps tried, steps accepted.  A sample with no point taking part at the start: R = I, t = 0, cost 0, info 0.
 *   Optional (NULL: skipped): normal_out [B][56] doubles = the start pose's 28 sums (H's upper triangle row-major, b, cost, each
 *   divided by n_used) and the same 28 sums over the terms' magnitudes; pose64_out [B][12] doubles = R and t unrounded.
 *   Checked before any launch (HOISDF_ERR_INVALID, the argument named in hoisdf_last_error): a required pointer null (values,
 *   grid, points, rot, trans, points_out, cost, info, workspace), B < 0 or > 65535, n, iters, V out of range, ld < n^3, huber not
 *   > 0, a negative lambda0 or step_tol, min_used_percent outside 0 .. 100, a workspace below
 *   hoisdf_field_fit_workspace_bytes(B) device bytes (-1 on an invalid B) or not aligned to 8 bytes.  B = 0 returns 0 with nothing
 *   launched.  The workspace holds the per-sample state in fp64 (pivot, extent, R, t, lambda, the 28 current sums, the trial
 *   pose, the counters, a status word); nothing in it needs to survive the call. */
#define HOISDF_FIELD_FIT_MAX_ITERS 64
long hoisdf_field_fit_workspace_bytes(int B);
int hoisdf_field_fit_launch_count(int iters);
int hoisdf_field_fit(const float* values, long ld, const float* grid, int n, const float* points, int V, const int32_t* n_points,
                     const float* pivot, int B, int iters, float huber, float lambda0, float step_tol, int min_used_percent,
                     float* rot, float* trans, float* points_out, double* cost, int32_t* info, double* normal_out,
                     double* pose64_out, void* workspace, long workspace_bytes, void* stream);

/* ---- raster: which pixels the posed hand mesh and the posed object mesh cover - ids, depth, modal masks, overlays, silhouette IoU ----
 * reference: none - the reference reads its masks from per-frame image files and never renders a mesh.  csrc/raster.hip;
 * hoisdf_amd/raster_oracle.py restates the rules below in numpy and reproduces every output bit for bit.  A z-buffered triangle
 * rasteriser with exact integer coverage; no gradient, no shading, no anti-aliasing, no near-plane clipping.  The result does not
 * depend on traversal order: two calls give the same bits.
 * Every entry checks its arguments before any launch (HOISDF_ERR_INVALID, the argument named in hoisdf_last_error), returns 0
 *   with nothing launched for B = 0 (B <= 65535), and only enqueues on `stream`.
 *
 * hoisdf_raster_meshes (2 launches: a setup pass over the faces, the raster pass over the pixels).
 *   Inputs: hand, obj as hoisdf_mesh_sdf_rows takes them (n_faces clamped to 0 .. max_faces, face rows from there on never read),
 *   ONE frame, metres, z forward.  Either mesh may be NULL, both NULL is invalid.  Mesh id: 0 = hand, 1 = obj.  K [B][6] floats =
 *   the top two rows of the camera matrix (the skew and rotation terms of an augmented K' are honoured), the third row is taken
 *   as 0 0 1.  width, height in 1 .. HOISDF_RASTER_MAX_SIZE.  half_pixel = 0: pixel (px, py) is sampled at (px, py), the OpenCV
 *   convention of the labels; 1: at (px + 0.5, py + 0.5).  near: finite, > 0.
 *   Projection, per vertex: floats widened to fp64, no product fused into a sum:  u = ((K0 x + K1 y) + K2 z) / z,
 *   v = ((K3 x + K4 y) + K5 z) / z;  snapped to 1/256 pixel: X = rint(256 u), Y = rint(256 v), round half to even, as int32.
 *   Skipped-face rule: a face takes no part in anything when it names a vertex outside 0 .. V-1; or a corner coordinate is not
 *   finite; or a corner has z < near (NO clipping: a triangle that crosses the near plane is dropped whole); or a corner has
 *   |u| or |v| >= 16384 (the guard band: |X|, |Y| <= 2^22); or its doubled area A2 = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0), in int64,
 *   is 0.  No back-face culling (the hand is open at the wrist, templates need not be closed): a face with A2 < 0 has its
 *   corners 1 and 2 swapped before the rules below.
 *   Coverage, exact, in integers: the sample point of pixel (px, py) is (px', py') = (256 px + 128 half_pixel, 256 py + 128
 *   half_pixel).  Edge i is the edge opposite corner i, from corner a = i + 1 to corner b = i + 2 (mod 3), dx = Xb - Xa,
 *   dy = Yb - Ya; its edge function, an int64, is E = dx (py' - Ya) - dy (px' - Xa).  The pixel is covered when all three E > 0,
 *   or when some are 0 and every such edge is a left edge (dy < 0: the interior at larger x along the pixel row) or a top edge
 *   (dy = 0 and dx > 0: horizontal, the interior at larger y, y pointing down).  A sample point on an edge shared by two faces
 *   belongs to exactly one of them, a point on a shared vertex to exactly one face of the fan.
 *   Depth, perspective-correct, fp64, one order, nothing fused:  l_i = (double)E_i / (double)A2;
 *   invz = (l0 (1/z0) + l1 (1/z1)) + l2 (1/z2);  z_pix = (float)(1 / invz).
 *   Visibility: a pixel keeps the covering face with the smallest key (z_pix as float32, mesh id, face row), compared in that
 *   order: an exact depth tie goes to the hand, within one mesh to the lower face row.
 *   Outputs, all optional (NULL: skipped), one at least; every element of a given output is written:
 *     id_out     int32 [B][height][width]: -1 for background, else mesh << 16 | face row
 *     depth_out  float, same shape: z_pix, 0 for background
 *     hand_seg, obj_seg  float [B][hm_h][hm_w], 1.0 / 0.0: mask pixel (i, j) reads raster pixel (floor((i + .5) width / hm_w),
 *                floor((j + .5) height / hm_h)) - the NEAREST fold of hoisdf_image_crop, no full-size mask is written; they need
 *                hm_w, hm_h >= 1, width % hm_w == 0 and height % hm_h == 0 (hm_w, hm_h are ignored without a mask).  The masks are
 *                MODAL: a pixel where the object is in front is no hand pixel.
 *     counts     int32 [B][2]: visible pixels per mesh at raster resolution (integer sums)
 *   workspace: hoisdf_raster_workspace_bytes(B, hand max_faces, obj max_faces) device bytes (0 for a NULL mesh; -1 on an invalid
 *   shape), 256-byte aligned: one 64-byte record per face row.
 *   The raster pass is tile-major: a workgroup owns a HOISDF_RASTER_TILE x HOISDF_RASTER_TILE tile of one sample, each thread its
 *   pixels outright, and the sample's records pass through LDS in chunks of HOISDF_RASTER_CHUNK.
 * hoisdf_raster_overlay (1 launch): image_in, image_out u8 [B][height][width][3] on the device, id as id_out above; colour u8
 *   [2][3] on the HOST (hand, obj; read before the call returns); alpha an integer in 0 .. 256.  A covered pixel becomes
 *   (alpha colour[mesh][c] + (256 - alpha) in + 128) >> 8, a background pixel is copied.  image_out == image_in is allowed.
 * hoisdf_eval_silhouette (1 launch): four masks float [B][n] (n in 1 .. 2^24), a value > 0.5 is set; counts int32 [B][4] = hand
 *   intersection, hand union, object intersection, object union of predicted against ground truth.  Integer sums only: the IoU
 *   is the caller's division. */
#define HOISDF_RASTER_TILE 32
#define HOISDF_RASTER_CHUNK 256
#define HOISDF_RASTER_MAX_SIZE 4096
long hoisdf_raster_workspace_bytes(int B, int hand_max_faces, int obj_max_faces);
int hoisdf_raster_meshes(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const float* K, int B, int width, int height,
                         int half_pixel, float near, int32_t* id_out, float* depth_out, float* hand_seg, float* obj_seg,
                         int hm_w, int hm_h, int32_t* counts, void* workspace, long workspace_bytes, void* stream);
int hoisdf_raster_overlay(const int32_t* id, const uint8_t* image_in, uint8_t* image_out, const uint8_t* colour, int alpha,
                          int B, int width, int height, void* stream);
int hoisdf_eval_silhouette(const float* pred_hand, const float* pred_obj, const float* gt_hand, const float* gt_obj, int B, int n,
                           int32_t* counts, void* stream);

/* ---- silhouette loss: a mask's distance transform, and a projected point set held to a pair of mask maps, with gradients -----------
 * reference: none - the reference supervises masks only at its CNN decoder.  Mesh regressors (HMR's descendants, SMPLify-X) hold a
 * predicted mesh to a silhouette through the DISTANCE TRANSFORM of the target mask instead of a differentiable rasteriser: projected
 * vertices are pulled into the silhouette, the silhouette's pixels are pulled under a projected vertex.  csrc/silhouette_loss.hip;
 * hoisdf_amd/silhouette_loss_oracle.py restates the rules below in numpy.  Integers and fp64, no float atomics, every sum in one
 * order: two calls give the same bits; a batch equals its samples run one by one, bit for bit.
 * Every entry checks its arguments before any launch (HOISDF_ERR_INVALID, the argument named in hoisdf_last_error), returns 0 with
 *   nothing launched for B = 0 (0 <= B <= 65535), and only enqueues on `stream`.  w, h in 1 .. HOISDF_EDT_MAX_SIZE.
 *
 * hoisdf_mask_edt (2 launches): the exact squared Euclidean distance transform.  mask, mask_or float [B][h][w], a value > 0.5 is set;
 *   mask_or may be NULL, otherwise the set is the union of the two ("hand or object").  Checked: mask or d2_out null, w, h, B.
 *     d2_out      int32 [B][h][w]: the squared distance in pixels^2 to the nearest set pixel of the sample, 0 at a set pixel,
 *                 HOISDF_EDT_NONE (= 2^30 = (2^15)^2) everywhere in a sample without a set pixel
 *     nearest_out int32, same shape, may be NULL: the index y' w + x' of a nearest set pixel, the LOWEST index on an exact tie; -1
 *                 in a sample without a set pixel
 *   Pass 1, one thread per column: g[y][x] = min |y - y'| over the set pixels of column x (the upper row on a tie), 2^15 for a
 *   column without one.  Pass 2, a workgroup per row with the row's g^2 in LDS: d2 = min over x' of min(g[y][x']^2 + (x - x')^2,
 *   HOISDF_EDT_NONE), every lane reading the same x'; ties by (y', x').  Integers only: no order dependence.  d2_out holds pass 1's
 *   rows in between: no workspace.
 *
 * hoisdf_silhouette_loss_fwd (3 launches) / _bwd (1 launch): ONE point set against ONE pair of maps (a caller with a hand and an
 *   object calls the pair twice).
 *   verts [B][V][3] camera frame, metres, z forward; n_verts [B] DEVICE int32 or NULL = V, clamped to 0 .. V: rows from n_verts[b]
 *   on are padding.  K [B][6] as hoisdf_raster_meshes takes it, but FOR THE MASK GRID: mask pixel (px, py) sits at (px, py).
 *   allow_d2 int32 [B][h][w]: a d2_out of hoisdf_mask_edt - where the points may lie.  cover float [B][h][w], set where > 0.5: the
 *   pixels the points must cover.  weight [V] floats per sample, may be NULL = all ones, weight_stride in elements 0 (one array
 *   shared by the batch) or V.  near: finite, > 0.
 *   Checked: verts, K, allow_d2, cover, an output or the workspace null; B; V < 1; w, h; near; a weight_stride that is neither 0 nor
 *   V; a workspace below hoisdf_silhouette_loss_workspace_bytes(B, V, w, h) device bytes (-1 on an invalid shape).
 *   Projection, per vertex: floats widened to fp64, no product fused into a sum:  u = ((K0 x + K1 y) + K2 z) / z,
 *   v = ((K3 x + K4 y) + K5 z) / z.  A vertex is INVALID when a coordinate is not finite, when z < near, when its row is >=
 *   n_verts[b], or when u or v is not finite: it takes no part in either term and gets zero gradient.
 *   Inside term, per valid vertex: uc = clamp(u, 0, w-1), vc = clamp(v, 0, h-1); x0 = min(floor(uc), w-2), y0 = min(floor(vc), h-2)
 *   (w = 1: x0 = 0 and the column weight fx is 0; h likewise); fx = uc - x0, fy = vc - y0; d = sqrt((double)allow_d2) at the four
 *   corners;  val = ((1-fx)(1-fy) d00 + fx (1-fy) d10) + ((1-fx) fy d01 + fx fy d11);  out = sqrt((u-uc)^2 + (v-vc)^2): a vertex
 *   that projects off the map is pulled back.  A corner with allow_d2 >= HOISDF_EDT_NONE (an empty allow mask) makes the vertex's
 *   term 0 with zero gradient.
 *     inside[b] = sum_v weight[v] (val + out) / sum_{v < n_verts[b]} weight[v]
 *   The denominator does not depend on the geometry; one that is not positive gives 0.
 *   Cover term, per set pixel p = (px, py) of cover: the nearest VALID vertex by dd = ((px-u)(px-u)) + ((py-v)(py-v)) in fp64, the
 *   lowest vertex index on an exact tie.
 *     cover_out[b] = sum_p sqrt(dd_p) / N_p,  N_p = the number of set pixels;  no set pixel, or no valid vertex, gives 0.
 *   Sums in fp64: thread t of 256 takes elements (vertices, pixels) t, t + 256, ... in ascending order, the 256 partial sums meet
 *   in the fixed tree s[t] += s[t + 128], s[t + 64], ... ; one rounding to fp32.
 *   Forward kernels: the projection; one workgroup per sample and tile of 256 pixels with the sample's (u, v) pairs passing
 *   through LDS, all lanes reading the same vertex, a wave without a set pixel skipping the scan; the per-sample reduction.
 *   workspace: 256-byte aligned pieces in this order, each rounded up to 256 bytes:  u double [B][V];  v double [B][V];  cell int32
 *   [B][V] = y0 w + x0, -1 for an invalid vertex;  nearest int32 [B][h w] = the nearest vertex of a set pixel, -1 for an unset
 *   pixel (or without a valid vertex);  den double [B][2] = the weight denominator, N_p.  hoisdf_silhouette_loss_bwd reads it, so
 *   between the two calls the workspace and every input stay as they were.
 *   Backward: upstream gradients g_inside, g_cover [B] (either may be NULL = zero) -> d_verts [B][V][3]; every row is written, a
 *   padding or invalid row gets 0.  Chain rule: du/dx = K0 / z, du/dy = K1 / z, du/dz = (K2 - u) / z, and likewise for v.
 *   Inside term: the bilinear derivative in fx, fy, zero along an axis that was clamped, plus the unit vector of (u-uc, v-vc) where
 *   out > 0, times weight / denominator times g_inside.  Cover term: vertex n receives (g_cover / N_p) ((u_n, v_n) - p) / sqrt(dd_p)
 *   from every set pixel whose nearest vertex it is; a pixel with dd_p = 0 contributes nothing.
 *   Order: no atomics; each vertex is owned by one lane, which adds in fp64, in (u, v), its own inside term first, then the pixels
 *   in ASCENDING pixel index (staged through LDS in tiles of HOISDF_SIL_LOSS_TILE records), applies the chain rule and rounds to
 *   fp32 once. */
#define HOISDF_EDT_MAX_SIZE 512
#define HOISDF_EDT_NONE 1073741824
#define HOISDF_SIL_LOSS_TILE 64
int hoisdf_mask_edt(const float* mask, const float* mask_or, int B, int w, int h, int32_t* d2_out, int32_t* nearest_out, void* stream);
long hoisdf_silhouette_loss_workspace_bytes(int B, int V, int w, int h);
int hoisdf_silhouette_loss_fwd(const float* verts, const int32_t* n_verts, int V, const float* K, int B,
                               const int32_t* allow_d2, const float* cover, int w, int h, float near,
                               const float* weight, long weight_stride,
                               float* inside, float* cover_out, void* workspace, long workspace_bytes, void* stream);
int hoisdf_silhouette_loss_bwd(const float* verts, const int32_t* n_verts, int V, const float* K, int B,
                               const int32_t* allow_d2, const float* cover, int w, int h, float near,
                               const float* weight, long weight_stride,
                               const float* g_inside, const float* g_cover,
                               float* d_verts, const void* workspace, long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOISDF_H_ */
