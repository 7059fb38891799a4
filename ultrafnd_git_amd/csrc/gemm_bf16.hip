// bf16 GEMM for the encoder Linears -- the product entry points (include/ultrafnd_hip.h).  Kernel, tile table and
// launcher: gemm_bf16_kernel.hpp.  No environment overrides, no ablation kernels, no stamps here: those live in
// diag/gemm_diag.hip (libultrafnd_hip_diag.so).
#include "gemm_bf16_kernel.hpp"
#include "gemm_bf16_checks.hpp"

// the persistent, software-pipelined form (gemm_bf16_pp.hpp), compiled in gemm_bf16_pp.hip
#define UFND_GEMM_TILE_PP UFND_GEMM_TILE_PERSISTENT
int ufnd_pp_pick(const void* gemm_args);
int ufnd_pp_launch(void* gemm_args, void* stream);
int ufnd_pp_stat_parts(int N);

namespace {
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* src, __bf16* dst, size_t n) {
  for (size_t i = (blockIdx.x * (size_t)256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
    if (i + 4 <= n) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
      bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<bf16x4*>(dst + i) = o;
    } else {
      for (size_t j = i; j < n; ++j) dst[j] = (__bf16)src[j];
    }
  }
}

}  // namespace

extern "C" int ufnd_gemm_bf16_live(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                                   float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                   int tile_cfg, const int* m_live, void* stream_) {
  int rc = gemm_bf16_check_args(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act);
  if (rc != UFND_OK) return rc;
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, residual, (__bf16*)out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, 0, 0, nullptr};
  a.m_live = m_live;
  if (tile_cfg == UFND_GEMM_TILE_PP || (tile_cfg < 0 && ufnd_pp_pick(&a))) return ufnd_pp_launch(&a, stream_);      // the persistent, software-pipelined form
  const int cfg = tile_cfg < 0 ? auto_cfg(M, N, K) : tile_cfg;
  rc = gemm_bf16_check_tile(cfg, N);
  if (rc != UFND_OK) return rc;
  rc = launch_cfg(cfg, 0, a, (hipStream_t)stream_);
  if (rc != UFND_OK) return rc;
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_gemm_bf16_ex(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                                 float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                 int tile_cfg, void* stream_) {
  return ufnd_gemm_bf16_live(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, tile_cfg, nullptr, stream_);
}

// A strided Conv1d over frames-as-rows (the audio feature extractor, csrc/audio.hip): the same kernel with an OVERLAPPING-row A
// operand, lda < K.  The kernel forms an A address as A + row * lda + k0 + 8 * chunk (issueA) and nothing else: no address
// computation uses lda as a bound on K, and a row index is clamped to M - 1, so the furthest element read is (M - 1) lda + K - 1,
// which the caller's buffer must hold.  The one-tile kernels only: the persistent form keeps 32-bit byte offsets sized for lda >= K
// operands and is not offered here.  Its own argument check -- the public GEMM entries keep requiring lda >= K.
extern "C" int ufnd_conv1d_rows_bf16(const void* A, const void* W, const float* bias, void* out_bf16, float* out_f32, int M, int N, int K, int lda,
                                     int ldw, int ldo, int ldf, int act, void* stream_) {
  UFND_REQUIRE(A && W && (out_bf16 || out_f32), "conv1d_rows: null operand");
  UFND_REQUIRE(M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "conv1d_rows: M=%d N=%d K=%d (need N%%64==0, K%%64==0)", M, N, K);
  UFND_REQUIRE(lda >= 8 && lda % 8 == 0 && ldw % 8 == 0 && ldw >= K && ufnd_aligned(A, 16) && ufnd_aligned(W, 16),
               "conv1d_rows: lda=%d ldw=%d (multiples of 8, ldw >= K) and 16-B aligned pointers", lda, ldw);
  UFND_REQUIRE((long long)M * lda + K < (1ll << 31), "conv1d_rows: M=%d lda=%d K=%d (the A operand must stay below 2^31 elements)", M, lda, K);
  UFND_REQUIRE(!out_f32 || (ldf % 4 == 0 && ldf >= N && ufnd_aligned(out_f32, 16)), "conv1d_rows: out_f32 alignment");
  UFND_REQUIRE(!out_bf16 || (ldo % 8 == 0 && ldo >= N && ufnd_aligned(out_bf16, 16)), "conv1d_rows: out_bf16 alignment");
  UFND_REQUIRE(!bias || ufnd_aligned(bias, 4), "conv1d_rows: bias alignment");
  UFND_REQUIRE(act >= 0 && act <= 2, "conv1d_rows: act=%d", act);
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, nullptr, (__bf16*)out_bf16, out_f32, M, N, K, lda, ldw, 0, ldo, ldf, act, 0, 0, nullptr};
  const int cfg = auto_cfg(M, N, K);
  int rc = gemm_bf16_check_tile(cfg, N);
  if (rc != UFND_OK) return rc;
  rc = launch_cfg(cfg, 0, a, (hipStream_t)stream_);
  if (rc != UFND_OK) return rc;
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_gemm_bf16_tile_info(int tile_cfg, int* bm, int* bn, int* ln_aware) {
  if (tile_cfg < 0 || tile_cfg >= kNumTiles || !kTiles[tile_cfg].built) return 0;
  if (bm) *bm = kTiles[tile_cfg].bm;
  if (bn) *bn = kTiles[tile_cfg].bn;
  if (ln_aware) *ln_aware = kTiles[tile_cfg].lnx;
  return 1;
}
extern "C" int ufnd_gemm_bf16_tile_count(void) { return kNumTiles; }

extern "C" int ufnd_gemm_bf16_stat_parts(int M, int N, int K) {
  // the automatic choice of an out_stats call on the bf16 residual stream (ufnd_gemm_ln.residual_bf16, bf16 output only) can be the
  // persistent form (pp_pick: the configs[3] geometry's out-projection, 65,536 rows): ask the same dispatch the call will take
  static const __bf16 probe[8] = {};
  GemmArgs a{};
  a.A = a.W = probe;
  a.out_bf16 = const_cast<__bf16*>(probe);
  a.residual_b = probe;
  a.out_stats = reinterpret_cast<float*>(const_cast<__bf16*>(probe));
  a.M = M; a.N = N; a.K = K; a.lda = a.ldw = K; a.ldo = a.ldrb = N;
  if (ufnd_pp_pick(&a)) return ufnd_pp_stat_parts(N);
  return stat_parts_for(auto_cfg(M, N, K), N);
}

extern "C" int ufnd_gemm_bf16_ln_live(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                                      float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                      const ufnd_gemm_ln* ln, const int* m_live, void* stream_) {
  int rc = gemm_bf16_ln_check_args(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, ln);
  if (rc != UFND_OK) return rc;
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, residual, (__bf16*)out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, 0, 0, nullptr};
  a.a_stats = ln->a_stats; a.colsum = ln->colsum; a.r_stats = ln->r_stats; a.r_gamma = ln->r_gamma; a.r_beta = ln->r_beta;
  a.out_stats = ln->out_stats; a.a_parts = ln->a_parts; a.r_parts = ln->r_parts; a.a_eps = ln->a_eps; a.r_eps = ln->r_eps;
  a.inv_h = 1.0f / (float)ln->width;
  a.residual_b = (const __bf16*)ln->residual_bf16;
  a.ldrb = ln->ldrb;
  a.guard = ln->a_stats ? ln->guard : nullptr;
  a.m_live = m_live;
  if (ln->tile_cfg == UFND_GEMM_TILE_PP || (ln->tile_cfg < 0 && ufnd_pp_pick(&a))) return ufnd_pp_launch(&a, stream_);      // the persistent, software-pipelined form
  const int cfg = ln->tile_cfg < 0 ? auto_cfg(M, N, K) : ln->tile_cfg;
  rc = gemm_bf16_ln_check_tile(cfg, M, N, K, ln);
  if (rc != UFND_OK) return rc;
  rc = launch_cfg(cfg, 4, a, (hipStream_t)stream_);
  if (rc != UFND_OK) return rc;
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_gemm_bf16_ln(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                                 float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                 const ufnd_gemm_ln* ln, void* stream_) {
  return ufnd_gemm_bf16_ln_live(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, ln, nullptr, stream_);
}

// BertSelfAttention of one layer in ONE launch: fused Q/K/V projection (optionally of LayerNorm(X), folded) + attention.
// bins / nbins (with cu_seqlens; ufnd_text_pack_bins): workgroup row tm runs bin tm's four 32-row slots, tm < *nbins
// (checks and launch arguments of the three geometries: gemm_bf16_checks.hpp)
extern "C" int ufnd_qkv_attention_bf16_bins(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask,
                                            const int32_t* cu_seqlens, const int32_t* bins, const int32_t* nbins, void* ctx, int B,
                                            int L, int heads, int ldx, int ldw, const ufnd_gemm_ln* ln, void* stream_) {
  GemmArgs a;
  const int rc = qkv_attention_pair_setup(a, X, Wqkv, bqkv, key_mask, cu_seqlens, bins, nbins, ctx, B, L, heads, ldx, ldw, ln);
  if (rc != UFND_OK) return rc;
  qkv_attention_launch<128, 384, 2, 4, 1, 0>(a, (hipStream_t)stream_);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_qkv_attention_bf16_packed(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask,
                                              const int32_t* cu_seqlens, void* ctx, int B, int L, int heads, int ldx, int ldw,
                                              const ufnd_gemm_ln* ln, void* stream_) {
  return ufnd_qkv_attention_bf16_bins(X, Wqkv, bqkv, key_mask, cu_seqlens, nullptr, nullptr, ctx, B, L, heads, ldx, ldw, ln, stream_);
}

extern "C" int ufnd_qkv_attention_bf16(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask, void* ctx,
                                       int B, int L, int heads, int ldx, int ldw, const ufnd_gemm_ln* ln, void* stream_) {
  return ufnd_qkv_attention_bf16_packed(X, Wqkv, bqkv, key_mask, nullptr, ctx, B, L, heads, ldx, ldw, ln, stream_);
}

// The packed form over sample tiles (ufnd_text_pack_tiles): one workgroup per (256-row tile of whole samples, head)
extern "C" int ufnd_qkv_attention_bf16_tiles(const void* X, const void* Wqkv, const float* bqkv, const int32_t* tiles, const int32_t* ntiles,
                                             void* ctx, int cap_tiles, int heads, int ldx, int ldw, const ufnd_gemm_ln* ln, void* stream_) {
  GemmArgs a;
  const int rc = qkv_attention_tiles_setup(a, X, Wqkv, bqkv, tiles, ntiles, ctx, cap_tiles, heads, ldx, ldw, ln);
  if (rc != UFND_OK) return rc;
  qkv_attention_launch<256, 192, 4, 2, 2, 0>(a, (hipStream_t)stream_);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// The same for samples of T <= 64 rows (CLIPAttention of a ViT layer: T = 50): one workgroup per (256 / T whole samples, head).
extern "C" int ufnd_qkv_attention_bf16_vit(const void* X, const void* Wqkv, const float* bqkv, void* ctx, int N, int T, int heads, int ldx,
                                           int ldw, const ufnd_gemm_ln* ln, void* stream_) {
  GemmArgs a;
  const int rc = qkv_attention_vit_setup(a, X, Wqkv, bqkv, ctx, N, T, heads, ldx, ldw, ln);
  if (rc != UFND_OK) return rc;
  qkv_attention_launch<256, 192, 4, 2, 1, 0>(a, (hipStream_t)stream_);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_gemm_bf16(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                              float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                              void* stream_) {
  return ufnd_gemm_bf16_ex(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, -1, stream_);
}

extern "C" int ufnd_cast_bf16(const float* src, void* dst, size_t n, void* stream_) {
  UFND_REQUIRE(src && dst && n > 0, "cast_bf16: null argument");
  UFND_REQUIRE(ufnd_aligned(src, 16) && ufnd_aligned(dst, 8), "cast_bf16: alignment");
  size_t want = (n / 4 + 255) / 256;
  const int blocks = (int)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, src, (__bf16*)dst, n);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
