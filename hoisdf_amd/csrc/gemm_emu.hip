// Host side of the fp32-emulating linear layers (hoisdf_linear_*_emu*): the process-wide form switch, the magnitude passes and their
// scratch, argument checks and the C entries.  The kernels and their launchers: gemm_emu_b3.hip (bf16x3 forward / grad-input),
// gemm_emu_h2.hip (f16x2 forward / grad-input), gemm_emu_dw.hip (grad-weight); shared declarations: gemm_emu.h.
#include <stdlib.h>

#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>

#include "gemm_emu.h"

namespace hoisdf {

// row magnitudes (common.h) of a row-major f32 matrix measured by the library: one wave per row, eight rows in flight per wave, plain
// stores (every row is written: no zeroing needed).  K % 4 == 0, rows 16-byte aligned.
__global__ __launch_bounds__(256) void emu_rowmag_kernel(const float* __restrict__ x, long ld, long M, int K, uint32_t* __restrict__ words) {
  constexpr int RPW = 8;
  const int lane = threadIdx.x & 63;
  const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  const int k4 = K >> 2;
  uint32_t m[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    m[r] = 0u;
    if (row0 + r < M)
      for (int c = lane; c < k4; c += 64) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(x + (row0 + r) * ld + 4 * c);
        m[r] = max(m[r], max(max(v[0] & 0x7fffffffu, v[1] & 0x7fffffffu), max(v[2] & 0x7fffffffu, v[3] & 0x7fffffffu)));
      }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const uint32_t mm = group_max_u32<64>(m[r]);
    if (lane == 0 && row0 + r < M) words[row0 + r] = mm;
  }
}
// head magnitudes (common.h) of a row-major f32 matrix: groups of 64 columns x samples of L rows -> words[group * nb + sample] (zero on
// entry).  One wave per 16 consecutive rows; a 16-lane group owns a column group (ncols = 64 groups: (groups + 3) / 4 sweeps).
__global__ __launch_bounds__(256) void emu_headmag_kernel(const float* __restrict__ x, long ld, long M, int groups, int L, int nb,
                                                          uint32_t* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  for (int g0 = 0; g0 < groups; g0 += 4) {
    const int grp = g0 + (lane >> 4);
    uint32_t m = 0u; long cur = -1;
    for (int r = 0; r < 16; ++r) {
      const long row = row0 + r;
      if (row >= M) break;
      const long b = row / L;
      if (b != cur) {
        if (cur >= 0 && grp < groups) { const uint32_t mm = group_max_u32<16>(m); if ((lane & 15) == 0) atomicMax(words + (size_t)grp * nb + cur, mm); }
        cur = b; m = 0u;
      }
      if (grp < groups) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(x + row * ld + grp * 64 + 4 * (lane & 15));
        m = max(m, max(max(v[0] & 0x7fffffffu, v[1] & 0x7fffffffu), max(v[2] & 0x7fffffffu, v[3] & 0x7fffffffu)));
      }
    }
    if (cur >= 0 && grp < groups) { const uint32_t mm = group_max_u32<16>(m); if ((lane & 15) == 0) atomicMax(words + (size_t)grp * nb + cur, mm); }
  }
}

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// HOISDF_EMU_FORM: "h2" (default) = the f16x2 form, "b3" = bf16x3 (six products).  Process-wide: it fixes the weight-image format.
bool form_h2() {
  static int f = -1;
  if (f < 0) { const char* e = getenv("HOISDF_EMU_FORM"); f = (e && (e[0] == 'b' || e[0] == 'B')) ? 0 : 1; }
  return f == 1;
}

}  // namespace

// row / head magnitudes for an operand nobody described: stream-ordered scratch from one arena per (device, stream) - the stream
// handle alone is not a key (torch's default stream is handle 0 on every device).  Everything that reads a slot runs on the slot's
// stream behind the pass that filled it, so wrapping around is safe whatever the arena's size; an arena that is too small for a
// request is replaced by a larger one (the old one stays allocated: launches in flight may still read it).  The first use on a
// stream allocates (hipMalloc synchronises and is illegal under graph capture: hosts that capture pass their own words).
uint32_t* mag_scratch(hipStream_t st, long words) {
  struct Arena { char* base = nullptr; size_t cap = 0, off = 0; };
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, Arena> arenas;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const size_t bytes = ((size_t)(words > 0 ? words : 1) * 4 + 255) & ~(size_t)255;
  std::lock_guard<std::mutex> lk(mu);
  Arena& a = arenas[std::make_pair(dev, st)];
  if (!a.base || bytes * 4 > a.cap) {
    const size_t cap = bytes * 8 > ((size_t)32 << 20) ? bytes * 8 : ((size_t)32 << 20);
    char* p = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&p), cap) != hipSuccess) return nullptr;
    a.base = p; a.cap = cap; a.off = 0;
  }
  if (a.off + bytes > a.cap) a.off = 0;
  uint32_t* r = reinterpret_cast<uint32_t*>(a.base + a.off);
  a.off += bytes;
  return r;
}

// HOISDF_MAG_TRACE=1: every operand the library had to measure itself, on stderr (who asked, rows x columns) - which producers to teach
static void mag_trace(const char* who, long M, int K) {
  static int on = -1;
  if (on < 0) { const char* e = getenv("HOISDF_MAG_TRACE"); on = (e && atoi(e) != 0) ? 1 : 0; }
  if (on) fprintf(stderr, "[hoisdf mag] measured by the library: %s operand %ld x %d\n", who, M, K);
}
// row magnitudes of a row-major matrix into `words` (M words, every one written)
int emu_rowmag_launch(const float* x, long ld, long M, int K, uint32_t* words, hipStream_t st) {
  if (M <= 0) return HOISDF_OK;
  hipLaunchKernelGGL(emu_rowmag_kernel, dim3((unsigned)cdiv(M, 32)), dim3(256), 0, st, x, ld, M, K, words);
  return check_launch("emu_rowmag");
}
// the same pass for an operand several contractions will read
int emu_mag_measure(const float* x, long ld, long M, int K, uint32_t* words, hipStream_t st) {
  mag_trace("a chain, once for all its readers:", M, K);
  return emu_rowmag_launch(x, ld, M, K, words, st);
}
// head magnitudes (common.h) of x[M][groups * 64 ...]: words[group * nb + row / L], nb = ceil(M / L); cleared here
int emu_headmag_launch(const float* x, long ld, long M, int groups, int L, uint32_t* words, hipStream_t st) {
  const int nb = cdiv(M, L);
  if (hipMemsetAsync(words, 0, (size_t)groups * nb * 4, st) != hipSuccess) { set_error("head magnitudes: memset failed"); return HOISDF_ERR_LAUNCH; }
  if (M <= 0) return HOISDF_OK;
  hipLaunchKernelGGL(emu_headmag_kernel, dim3((unsigned)cdiv(M, 64)), dim3(256), 0, st, x, ld, M, groups, L, nb, words);
  return check_launch("emu_headmag");
}
bool emu_form_h2() { return form_h2(); }
// may the GEMM epilogue fold the head magnitudes of its output?  Its unit is the wave's 128-row sub-tile: exact only when every
// sub-tile lies inside one sample and holds no rows past M (those carry the bias).  Otherwise the words are measured on the stored
// matrix (emu_headmag_launch): a sample's scale must not depend on its batch neighbours.
static bool heads_fold_exact(long M, int head_L) { return head_L % 128 == 0 && M % 128 == 0; }

namespace {
int launch_emu(EmuArgs g, hipStream_t st) {
  g.vecC = al16(g.C) && (g.ldc % 4 == 0);
  if (g.beta) g.amax_out = nullptr;           // (the tile is added to what is there: its own magnitude says nothing)
  if (!form_h2()) return emu_b3_launch(g, st);
  if (!g.a_amax) {
    uint32_t* part = mag_scratch(st, g.M);
    if (!part) { set_error("linear_emu: cannot allocate the row magnitudes"); return HOISDF_ERR_LAUNCH; }
    mag_trace(g.beta ? "grad-input (+=)" : g.abits ? "grad-input (masked)" : g.qkv.on ? "in-projection" : "forward / grad-input", g.M, g.K);
    if (int rc = emu_rowmag_launch(g.A, g.lda, g.M, g.K, part, st)) return rc;
    g.a_amax = part;
  }
  return emu_h2_launch(g, st);
}
}  // namespace

}  // namespace hoisdf

using namespace hoisdf;

extern "C" long hoisdf_linear_emu_image_bytes(int rows, int K) {
  if (rows <= 0 || K <= 0) return 0;
  if (form_h2()) return (long)cdiv(rows, HTN) * cdiv(K, KS) * HB_U4 * 16 + H_TRAILER;
  return (long)cdiv(rows, TN) * cdiv(K, KS) * B_U4 * 16;
}

extern "C" int hoisdf_linear_emu_prepare(const float* W, int ldw, int N, int K, int transpose, void* image, void* stream) {
  HOISDF_REQUIRE(W && image && N > 0 && K > 0 && ldw >= K, HOISDF_ERR_INVALID, "linear_emu_prepare: bad arguments");
  HOISDF_REQUIRE(al16(image), HOISDF_ERR_INVALID, "linear_emu_prepare: the image must be 16-byte aligned");
  if (form_h2()) return emu_h2_prepare(W, ldw, N, K, transpose, image, as_stream(stream));
  return emu_b3_prepare(W, ldw, transpose ? K : N, transpose ? N : K, transpose, image, as_stream(stream));
}

extern "C" long hoisdf_linear_emu_prepare_blocks(int N, int K, int transpose) {
  if (N <= 0 || K <= 0) return 0;
  const int R = transpose ? K : N, Kc = transpose ? N : K;
  if (form_h2()) return ((long)cdiv(R, HTN) * cdiv(Kc, KS) * 2 * HTN + 255) / 256;
  return ((long)cdiv(R, TN) * cdiv(Kc, KS) * 2 * TN + 255) / 256;
}

extern "C" int hoisdf_linear_emu_prepare_batch(const hoisdf_emu_prep_item* d_items, int n, long total_blocks, void* stream) {
  HOISDF_REQUIRE(n >= 0 && total_blocks >= 0 && total_blocks < (1L << 31), HOISDF_ERR_INVALID, "linear_emu_prepare_batch: bad sizes");
  if (n == 0 || total_blocks == 0) return HOISDF_OK;
  HOISDF_REQUIRE(d_items, HOISDF_ERR_INVALID, "linear_emu_prepare_batch: null table");
  return (form_h2() ? emu_h2_prepare_batch : emu_b3_prepare_batch)(d_items, n, total_blocks, as_stream(stream));
}

extern "C" int hoisdf_linear_emu_supported(const float* a, long lda, int Kc) {
  return a && al16(a) && (lda % 4 == 0) && (Kc % 4 == 0) && Kc >= 4;
}

extern "C" int hoisdf_linear_fwd_emu(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M,
                                     int N, int K, int act, float drop_p, uint64_t seed, uint32_t* relu_bits, void* stream) {
  return linear_fwd_emu_mag(x, ldx, w_image, bias, y, ldy, M, N, K, act, drop_p, seed, relu_bits, nullptr, nullptr, stream);
}
extern "C" int hoisdf_linear_fwd_emu_mag(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M,
                                         int N, int K, int act, float drop_p, uint64_t seed, uint32_t* relu_bits, const uint32_t* x_mag,
                                         uint32_t* y_mag, void* stream) {
  return linear_fwd_emu_mag(x, ldx, w_image, bias, y, ldy, M, N, K, act, drop_p, seed, relu_bits, x_mag, y_mag, stream);
}
// row magnitudes (include/hoisdf.h): u32 words a matrix of `rows` rows takes
extern "C" long hoisdf_mag_words(long rows) { return rows > 0 ? rows : 0; }
// the row magnitudes of a matrix nobody left words for: one read of x (hosts that chain the *_mag entries themselves call this once per
// operand instead of letting every contraction measure it again); every word is written, no clearing needed
extern "C" int hoisdf_mag_measure(const float* x, long ldx, long M, int K, uint32_t* words, void* stream) {
  HOISDF_REQUIRE(words && (M == 0 || x) && M >= 0 && K > 0 && ldx >= K, HOISDF_ERR_INVALID, "mag_measure: bad arguments");
  HOISDF_REQUIRE(M == 0 || hoisdf_linear_emu_supported(x, ldx, K), HOISDF_ERR_INVALID, "mag_measure: x must be 16-byte aligned with ldx and K multiples of 4");
  return emu_rowmag_launch(x, ldx, M, K, words, as_stream(stream));
}
// head magnitudes (include/hoisdf.h) of an attention operand matrix x[M][>= groups * 64], samples of L rows: words a host must provide,
// and the pass that fills them (clears first)
extern "C" long hoisdf_head_mag_words(long M, int groups, int L) { return (M > 0 && groups > 0 && L > 0) ? (long)groups * cdiv(M, L) : 0; }
extern "C" int hoisdf_head_mag_measure(const float* x, long ldx, long M, int groups, int L, uint32_t* words, void* stream) {
  HOISDF_REQUIRE(words && (M == 0 || x) && M >= 0 && groups > 0 && L > 0 && ldx >= (long)groups * 64 && ldx % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(x) & 15) == 0, HOISDF_ERR_INVALID, "head_mag_measure: bad arguments");
  return emu_headmag_launch(x, ldx, M, groups, L, words, as_stream(stream));
}
extern "C" int hoisdf_linear_emu_pieces(void) { return form_h2() ? 2 : 3; }

int hoisdf::linear_fwd_emu_mag(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M, int N, int K,
                               int act, float drop_p, uint64_t seed, uint32_t* relu_bits, const uint32_t* x_mag, uint32_t* y_mag,
                               void* stream, uint32_t* y_heads, int head_L) {
  HOISDF_REQUIRE(M == 0 || (x && w_image && y), HOISDF_ERR_INVALID, "linear_fwd_emu: null pointer");
  HOISDF_REQUIRE(M >= 0 && N > 0 && K > 0 && ldx >= K && ldy >= N && M < (1L << 31), HOISDF_ERR_INVALID,
                 "linear_fwd_emu: bad sizes M=%ld N=%d K=%d ldx=%d ldy=%d", M, N, K, ldx, ldy);
  HOISDF_REQUIRE(drop_p >= 0.f && drop_p < 1.f, HOISDF_ERR_INVALID, "linear_fwd_emu: drop_p=%f", drop_p);
  if (M == 0) return HOISDF_OK;
  HOISDF_REQUIRE(hoisdf_linear_emu_supported(x, ldx, K), HOISDF_ERR_INVALID,
                 "linear_fwd_emu: x must be 16-byte aligned with ldx and K multiples of 4 (use hoisdf_linear_fwd otherwise)");
  EmuArgs g{};
  g.A = x; g.lda = ldx; g.Bimg = static_cast<const u32x4*>(w_image);
  g.C = y; g.ldc = ldy; g.bias = bias; g.M = (int)M; g.N = N; g.K = K;
  g.act = act; g.drop_p = drop_p; g.inv_keep = 1.f / (1.f - drop_p); g.thresh = drop_threshold(drop_p); g.seed = seed;
  g.bits_out = relu_bits; g.ldbits_out = (N + 31) / 32;
  g.a_amax = x_mag; g.amax_out = y_mag;
  bool measure_heads = false;
  if (y_heads) {
    HOISDF_REQUIRE(head_L > 0 && N % 64 == 0, HOISDF_ERR_INVALID, "linear_fwd_emu: head magnitudes need N %% 64 == 0 and the rows per sample");
    if (heads_fold_exact(M, head_L)) { g.head_out = y_heads; g.head_L = head_L; g.head_nb = cdiv(M, head_L); }
    else {
      HOISDF_REQUIRE(al16(y) && ldy % 4 == 0, HOISDF_ERR_INVALID, "linear_fwd_emu: head magnitudes of samples that are no multiple of 128 rows need y 16-byte aligned, ldy %% 4 == 0");
      measure_heads = true;
    }
  }
  if (int rc = launch_emu(g, as_stream(stream))) return rc;
  // samples that share 128-row sub-tiles: the words of the stored y, one more read of it (what hoisdf_head_mag_measure gives)
  return measure_heads ? emu_headmag_launch(y, ldy, M, N / 64, head_L, y_heads, as_stream(stream)) : HOISDF_OK;
}

// hoisdf_linear_fwd_emu whose output goes into attention planes (common.h QkvPlanes; internal: the coarse layer entries use it)
int hoisdf::linear_fwd_emu_qkv(const float* x, int ldx, const void* w_image, const float* bias, long M, int N, int K,
                               const QkvPlanes& pl, void* stream, const uint32_t* x_mag) {
  HOISDF_REQUIRE(x && w_image && M > 0 && N > 0 && K > 0 && ldx >= K && M < (1L << 31), HOISDF_ERR_INVALID, "linear_fwd_emu_qkv: bad arguments");
  HOISDF_REQUIRE(hoisdf_linear_emu_supported(x, ldx, K), HOISDF_ERR_INVALID, "linear_fwd_emu_qkv: x alignment / K");
  HOISDF_REQUIRE(pl.on && pl.L > 0 && pl.L % 128 == 0 && M % pl.L == 0 && N % 64 == 0 && pl.E % 64 == 0 && pl.Lp >= pl.L &&
                     pl.col0 % 64 == 0 && pl.col0 + N <= 3 * pl.E,
                 HOISDF_ERR_INVALID, "linear_fwd_emu_qkv: plane geometry (L=%d Lp=%d N=%d E=%d col0=%d)", pl.L, pl.Lp, N, pl.E, pl.col0);
  EmuArgs g{};
  g.A = x; g.lda = ldx; g.Bimg = static_cast<const u32x4*>(w_image);
  g.C = nullptr; g.ldc = N; g.bias = bias; g.M = (int)M; g.N = N; g.K = K;
  g.inv_keep = 1.f; g.qkv = pl;
  g.a_amax = x_mag;
  return launch_emu(g, as_stream(stream));
}

extern "C" int hoisdf_linear_fwd_emu_heads(const float* x, int ldx, const void* w_image, const float* bias, float* y, int ldy, long M, int N,
                                           int K, const uint32_t* x_mag, uint32_t* y_mag, uint32_t* y_heads, int L, void* stream) {
  HOISDF_REQUIRE(y_heads, HOISDF_ERR_INVALID, "linear_fwd_emu_heads: y_heads is required");
  return linear_fwd_emu_mag(x, ldx, w_image, bias, y, ldy, M, N, K, 0, 0.f, 0, nullptr, x_mag, y_mag, stream, y_heads, L);
}
extern "C" int hoisdf_linear_bwd_input_emu_heads(const float* dy, int lddy, const void* wt_image, float* dx, int lddx, long M, int N, int K,
                                                 const uint32_t* dy_mag, uint32_t* dx_mag, uint32_t* dx_heads, int L, void* stream) {
  HOISDF_REQUIRE(dx_heads, HOISDF_ERR_INVALID, "linear_bwd_input_emu_heads: dx_heads is required");
  return linear_bwd_input_emu_mag(dy, lddy, nullptr, 0.f, wt_image, dx, lddx, M, N, K, 0, dy_mag, dx_mag, stream, dx_heads, L);
}
extern "C" int hoisdf_linear_bwd_input_emu(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p,
                                           const void* wt_image, float* dx, int lddx, long M, int N, int K, int accumulate,
                                           void* stream) {
  return linear_bwd_input_emu_mag(dy, lddy, relu_bits, drop_p, wt_image, dx, lddx, M, N, K, accumulate, nullptr, nullptr, stream);
}
extern "C" int hoisdf_linear_bwd_input_emu_mag(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p,
                                               const void* wt_image, float* dx, int lddx, long M, int N, int K, int accumulate,
                                               const uint32_t* dy_mag, uint32_t* dx_mag, void* stream) {
  return linear_bwd_input_emu_mag(dy, lddy, relu_bits, drop_p, wt_image, dx, lddx, M, N, K, accumulate, dy_mag, dx_mag, stream);
}

int hoisdf::linear_bwd_input_emu_mag(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const void* wt_image, float* dx,
                                     int lddx, long M, int N, int K, int accumulate, const uint32_t* dy_mag, uint32_t* dx_mag,
                                     void* stream, uint32_t* dx_heads, int head_L) {
  HOISDF_REQUIRE(M == 0 || (dy && wt_image && dx), HOISDF_ERR_INVALID, "linear_bwd_input_emu: null pointer");
  HOISDF_REQUIRE(M >= 0 && N > 0 && K > 0 && lddy >= N && lddx >= K && M < (1L << 31) && drop_p >= 0.f && drop_p < 1.f,
                 HOISDF_ERR_INVALID, "linear_bwd_input_emu: bad sizes");
  if (M == 0) return HOISDF_OK;
  HOISDF_REQUIRE(hoisdf_linear_emu_supported(dy, lddy, N), HOISDF_ERR_INVALID,
                 "linear_bwd_input_emu: dy must be 16-byte aligned with lddy and N multiples of 4");
  EmuArgs g{};
  // dx[m][k] = sum_n dy[m][n] W[n][k]: A = dy rows (contraction n contiguous), B = the transposed image ([k][n])
  g.A = dy; g.lda = lddy; g.Bimg = static_cast<const u32x4*>(wt_image);
  g.abits = relu_bits; g.ldbits = (N + 31) / 32; g.ascale = 1.f / (1.f - drop_p);
  g.C = dx; g.ldc = lddx; g.M = (int)M; g.N = K; g.K = N;
  g.inv_keep = 1.f;
  g.beta = accumulate ? 1 : 0;
  g.a_amax = dy_mag; g.amax_out = dx_mag;
  bool measure_heads = false;
  if (dx_heads) {
    HOISDF_REQUIRE(head_L > 0 && K % 64 == 0 && !accumulate, HOISDF_ERR_INVALID, "linear_bwd_input_emu: head magnitudes need K %% 64 == 0, the rows per sample, no accumulation");
    if (heads_fold_exact(M, head_L)) { g.head_out = dx_heads; g.head_L = head_L; g.head_nb = cdiv(M, head_L); }
    else {
      HOISDF_REQUIRE(al16(dx) && lddx % 4 == 0, HOISDF_ERR_INVALID, "linear_bwd_input_emu: head magnitudes of samples that are no multiple of 128 rows need dx 16-byte aligned, lddx %% 4 == 0");
      measure_heads = true;
    }
  }
  if (int rc = launch_emu(g, as_stream(stream))) return rc;
  return measure_heads ? emu_headmag_launch(dx, lddx, M, K / 64, head_L, dx_heads, as_stream(stream)) : HOISDF_OK;
}

extern "C" long hoisdf_linear_bwd_weight_emu_workspace(long M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int splitk, mper;
  plan_dw(M, N, K, splitk, mper);
  if (splitk <= 1) return 0;
  return (long)splitk * ((long)N * K + N);
}

namespace {
int bwd_weight_emu(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x, int ldx, float* dW, int lddw,
                   float* db, long M, int N, int K, float* workspace, long workspace_floats, bool h2, const uint32_t* dy_mag,
                   const uint32_t* x_mag, void* stream) {
  HOISDF_REQUIRE(dW && (M == 0 || (dy && x)), HOISDF_ERR_INVALID, "linear_bwd_weight_emu: null pointer");
  HOISDF_REQUIRE(M > 0 && N > 0 && K > 0 && lddy >= N && ldx >= K && lddw == K && M < (1L << 31) && drop_p >= 0.f && drop_p < 1.f,
                 HOISDF_ERR_INVALID, "linear_bwd_weight_emu: bad sizes (a dense dW, lddw == K, is required)");
  HOISDF_REQUIRE(al16(dy) && al16(x) && al16(dW) && (lddy % 4 == 0) && (ldx % 4 == 0) && (N % 4 == 0) && (K % 4 == 0),
                 HOISDF_ERR_INVALID, "linear_bwd_weight_emu: operands must be 16-byte aligned with N, K and leading dims multiples of 4");
  hipStream_t st = as_stream(stream);
  DwArgs g{};
  g.dy = dy; g.lddy = lddy; g.x = x; g.ldx = ldx;
  g.bits = relu_bits; g.ldbits = (N + 31) / 32; g.ascale = 1.f / (1.f - drop_p);
  g.M = (int)M; g.N = N; g.K = K;
  const int dtk = dw_tile(K);
  g.tiles_n = cdiv(N, DT); g.tiles_k = cdiv(K, dtk);
  plan_dw(M, N, K, g.splitk, g.m_per_split);
  const long need = g.splitk > 1 ? (long)g.splitk * ((long)N * K + N) : 0;
  HOISDF_REQUIRE(need == 0 || (workspace && workspace_floats >= need && al16(workspace)), HOISDF_ERR_WORKSPACE,
                 "linear_bwd_weight_emu: workspace of %ld floats needed", need);
  if (g.splitk > 1) {
    g.C = workspace; g.c_split_stride = (long)N * K;
    g.colsum = db ? workspace + (size_t)g.splitk * N * K : nullptr; g.colsum_split_stride = N;
  } else {
    g.C = dW; g.c_split_stride = 0; g.colsum = db; g.colsum_split_stride = 0;
  }
  if (dtk == 256 && h2) {
    g.dy_amax = dy_mag; g.x_amax = x_mag;
    if (!dy_mag) {
      uint32_t* part = mag_scratch(st, M);
      if (!part) { set_error("linear_bwd_weight_emu: cannot allocate the row magnitudes"); return HOISDF_ERR_LAUNCH; }
      mag_trace("grad-weight dy", M, N);
      if (int rc = emu_rowmag_launch(dy, lddy, M, N, part, st)) return rc;
      g.dy_amax = part;
    }
    if (!x_mag) {
      uint32_t* part = mag_scratch(st, M);
      if (!part) { set_error("linear_bwd_weight_emu: cannot allocate the row magnitudes"); return HOISDF_ERR_LAUNCH; }
      mag_trace("grad-weight x", M, K);
      if (int rc = emu_rowmag_launch(x, ldx, M, K, part, st)) return rc;
      g.x_amax = part;
    }
  }
  return emu_dw_launch(g, h2, dW, db, workspace, st);
}
}  // namespace

extern "C" int hoisdf_linear_bwd_weight_emu(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x,
                                            int ldx, float* dW, int lddw, float* db, long M, int N, int K, float* workspace,
                                            long workspace_floats, void* stream) {
  return bwd_weight_emu(dy, lddy, relu_bits, drop_p, x, ldx, dW, lddw, db, M, N, K, workspace, workspace_floats, false, nullptr, nullptr, stream);
}
// the f16x2 form (when the process runs it, hoisdf_linear_emu_pieces() == 2, and the tile is the 256-wide one; otherwise as above):
// dy_mag / x_mag = magnitude words of the two operands, NULL = measured here
int hoisdf::linear_bwd_weight_emu_mag(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x, int ldx,
                                      float* dW, int lddw, float* db, long M, int N, int K, float* workspace, long workspace_floats,
                                      const uint32_t* dy_mag, const uint32_t* x_mag, void* stream) {
  return bwd_weight_emu(dy, lddy, relu_bits, drop_p, x, ldx, dW, lddw, db, M, N, K, workspace, workspace_floats, form_h2(), dy_mag, x_mag, stream);
}
extern "C" int hoisdf_linear_bwd_weight_emu_mag(const float* dy, int lddy, const uint32_t* relu_bits, float drop_p, const float* x,
                                                int ldx, float* dW, int lddw, float* db, long M, int N, int K, float* workspace,
                                                long workspace_floats, const uint32_t* dy_mag, const uint32_t* x_mag, void* stream) {
  return linear_bwd_weight_emu_mag(dy, lddy, relu_bits, drop_p, x, ldx, dW, lddw, db, M, N, K, workspace, workspace_floats, dy_mag, x_mag, stream);
}
