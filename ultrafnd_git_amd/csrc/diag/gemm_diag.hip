// Diagnostics build of the bf16 GEMM (libultrafnd_hip_diag.so; never loaded by the product package): every tile of
// the table, the timing-only ablation kernels (no MFMA / no in-loop DMA: results are garbage), the in-kernel stamps
// build and the UFND_GEMM_FORCE_CFG override.  Used by tools/gemm_sweep.py and tools/gemm_stamps.py.
#define UFND_DIAG 1
#include "../gemm_bf16_kernel.hpp"
#include "../gemm_bf16_checks.hpp"

// out = act(A W^T + bias) + residual with an explicit tile; tile_cfg + 100 / + 200 select the timing-only ablations.
extern "C" int ufnd_diag_gemm_bf16_ex(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                                      float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                      int tile_cfg, void* stream_) {
  UFND_REQUIRE(A && W && (out_bf16 || out_f32), "diag gemm: null operand");
  UFND_REQUIRE(M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "diag gemm: M=%d N=%d K=%d", M, N, K);
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, residual, (__bf16*)out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, 0, 0, nullptr};
  int mode = 0, cfg = tile_cfg < 0 ? auto_cfg(M, N, K) : tile_cfg;
  if (cfg >= 200) { mode = 2; cfg -= 200; } else if (cfg >= 100) { mode = 1; cfg -= 100; }
  UFND_REQUIRE(cfg < kNumTiles, "diag gemm: unknown tile config %d", cfg);
  UFND_REQUIRE(N % kTiles[cfg].bn == 0, "diag gemm: tile config %d needs N %% %d == 0", cfg, kTiles[cfg].bn);
  int rc = launch_cfg(cfg, mode, a, (hipStream_t)stream_);
  if (rc != UFND_OK) return rc;
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// One launch of tile `tile_cfg` built with in-kernel clock stamps.  stamps receives 8 uint64 per block: {s_memtime,
// s_memrealtime} at kernel entry, after the first K-step has landed, after the K loop, after the last store has drained.
// ln != NULL times the LayerNorm-aware kernel of that tile (bias, residual, out_f32 as in ufnd_gemm_bf16_ln; strides = N).
extern "C" int ufnd_diag_gemm_bf16_stamps(const void* A, const void* W, void* out_bf16, int M, int N, int K, int tile_cfg,
                                     unsigned long long* stamps, const ufnd_gemm_ln* ln, const float* bias, const float* residual,
                                     float* out_f32, void* stream_) {
  UFND_REQUIRE(A && W && out_bf16 && stamps, "gemm_bf16_stamps: null operand");
  UFND_REQUIRE(M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "gemm_bf16_stamps: M=%d N=%d K=%d", M, N, K);
  UFND_REQUIRE(tile_cfg >= 0 && tile_cfg < kNumTiles && N % kTiles[tile_cfg].bn == 0, "gemm_bf16_stamps: tile config %d", tile_cfg);
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, residual, (__bf16*)out_bf16, out_f32, M, N, K, K, K, N, N, N, 0, 0, 0, stamps};
  int abl = 3;
  if (ln) {      // the LayerNorm-aware kernel of this tile, same extras as ufnd_gemm_bf16_ln (unchecked: diagnostics)
    UFND_REQUIRE(kTiles[tile_cfg].lnx, "gemm_bf16_stamps: tile %d has no LayerNorm-aware kernel", tile_cfg);
    a.a_stats = ln->a_stats; a.colsum = ln->colsum; a.r_stats = ln->r_stats; a.r_gamma = ln->r_gamma; a.r_beta = ln->r_beta;
    a.out_stats = ln->out_stats; a.a_parts = ln->a_parts; a.r_parts = ln->r_parts; a.a_eps = ln->a_eps; a.r_eps = ln->r_eps;
    a.inv_h = 1.0f / (float)ln->width;
    a.residual_b = (const __bf16*)ln->residual_bf16;      // bf16 residual stream (round 3)
    a.ldrb = ln->ldrb;
    a.guard = ln->a_stats ? ln->guard : nullptr;          // fold guard inside the GEMM (ABI v4)
    if (ln->tile_cfg > 0) a.act = ln->tile_cfg;           // (this entry takes the tile as an argument: the field carries the activation)
    abl = 5;
  }
  int rc = launch_cfg(tile_cfg, abl, a, (hipStream_t)stream_);
  if (rc != UFND_OK) return rc;
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// The fused projection + attention kernel with stamps: 10 uint64 per workgroup -- {s_memtime, s_memrealtime} at entry, first
// K-step landed, K loop done, END, and (slots 8, 9) projection epilogue done / attention starts.
extern "C" int ufnd_diag_qkv_attention_stamps(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask, void* ctx, int B,
                                              int heads, const ufnd_gemm_ln* ln, unsigned long long* stamps, void* stream_) {
  UFND_REQUIRE(stamps, "diag qkv_attention: null stamps");
  GemmArgs a;
  const int rc = qkv_attention_pair_setup(a, X, Wqkv, bqkv, key_mask, nullptr, nullptr, nullptr, ctx, B, 128, heads, heads * 64, heads * 64, ln);
  if (rc != UFND_OK) return rc;
  a.stamps = stamps;
  qkv_attention_launch<128, 384, 2, 4, 1, 1>(a, (hipStream_t)stream_);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// The same stamps for the sample-tile form (ufnd_qkv_attention_bf16_tiles over a table of ufnd_text_pack_tiles); 10 stamps per workgroup
// of the cap_tiles x heads grid, workgroups past *ntiles leave theirs untouched.
extern "C" int ufnd_diag_qkv_attention_tiles_stamps(const void* X, const void* Wqkv, const float* bqkv, const int32_t* tiles, const int32_t* ntiles,
                                                    void* ctx, int cap_tiles, int heads, const ufnd_gemm_ln* ln, unsigned long long* stamps,
                                                    void* stream_) {
  UFND_REQUIRE(stamps, "diag qkv_attention_tiles: null stamps");
  GemmArgs a;
  const int rc = qkv_attention_tiles_setup(a, X, Wqkv, bqkv, tiles, ntiles, ctx, cap_tiles, heads, heads * 64, heads * 64, ln);
  if (rc != UFND_OK) return rc;
  a.stamps = stamps;
  qkv_attention_launch<256, 192, 4, 2, 2, 1>(a, (hipStream_t)stream_);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// Validation, tile choice and launch geometry of one call of the product's one-tile entries, on the host only: nothing is launched
// and no operand is dereferenced -- the pointers only have to carry the alignment of the real ones -- so this answers on a machine
// without a GPU (tests/test_gemm_bf16_cases.py).  The argument checks are the product entries' own (gemm_bf16_checks.hpp), the
// choice is auto_cfg / xcd_cols_for / stat_parts_for as launch_cfg applies them.
//   entry  0 ufnd_gemm_bf16 (automatic tile), 1 ufnd_gemm_bf16_ex (tile_cfg), 2 ufnd_gemm_bf16_ln (ln->tile_cfg), 3 ufnd_gemm_bf16_dgrad;
//         -1: the table row of tile `tile_cfg` only (returns UFND_ERR_INVALID past the table's end)
//   out   {tile, m_tiles, n_tiles, xcd_cols, out_stats partials per row (0 without out_stats), bm, bn, A ring depth, W ring depth,
//          ln_aware, part of the product library, has a backward kernel}
// The persistent form (gemm_bf16_pp.hpp) is not planned here: its automatic choice reads the device's CU count.  A shape it could
// take (ufnd_diag_pp_shape_ok) is refused for the automatic forward entries, and so is UFND_GEMM_TILE_PERSISTENT.  Its own plan
// entry, which takes the CU count as an argument, is ufnd_diag_gemm_pp_plan (gemm_pp_diag.hip).
int ufnd_diag_pp_shape_ok(int M, int N, int K);      // gemm_pp_diag.hip
extern "C" int ufnd_diag_gemm_bf16_plan(int entry, const void* A, const void* W, const float* bias, const float* residual, const void* aux,
                                        const void* out_bf16, const float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldaux,
                                        int ldo, int ldf, int act, int tile_cfg, const ufnd_gemm_ln* ln, int* out) {
  UFND_REQUIRE(out, "gemm_bf16_plan: null result pointer");
  UFND_REQUIRE(entry >= -1 && entry <= 3, "gemm_bf16_plan: entry %d", entry);
  int cfg = tile_cfg, rc = UFND_OK, parts = 0;
  if (entry == -1) {
    UFND_REQUIRE(cfg >= 0 && cfg < kNumTiles, "gemm_bf16_plan: no tile %d", cfg);
    M = N = K = 0;
  } else if (entry == 3) {
    rc = gemm_bf16_dgrad_check_args(A, W, residual, aux, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldaux, ldo, ldf, act);
    if (rc != UFND_OK) return rc;
    cfg = auto_cfg(M, N, K);
    rc = gemm_bf16_dgrad_check_tile(cfg, N);
    if (rc != UFND_OK) return rc;
  } else {
    if (entry == 2) {
      rc = gemm_bf16_ln_check_args(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, ln);
      if (rc != UFND_OK) return rc;
      cfg = ln->tile_cfg;
    } else {
      rc = gemm_bf16_check_args(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act);
      if (rc != UFND_OK) return rc;
      if (entry == 0) cfg = -1;
    }
    UFND_REQUIRE(cfg != UFND_GEMM_TILE_PERSISTENT && !(cfg < 0 && ufnd_diag_pp_shape_ok(M, N, K)),
                 "gemm_bf16_plan: the persistent form may take this call (its choice needs the device): not planned here");
    if (cfg < 0) cfg = auto_cfg(M, N, K);
    rc = entry == 2 ? gemm_bf16_ln_check_tile(cfg, M, N, K, ln) : gemm_bf16_check_tile(cfg, N);
    if (rc != UFND_OK) return rc;
    if (entry == 2 && ln->out_stats) parts = stat_parts_for(cfg, N);
  }
  const TileCfg& t = kTiles[cfg];
  const int m_tiles = entry < 0 ? 0 : ufnd_cdiv(M, t.bm), n_tiles = entry < 0 ? 0 : N / t.bn;      // (as launch_cfg)
  out[0] = cfg;
  out[1] = m_tiles;
  out[2] = n_tiles;
  out[3] = entry < 0 ? 0 : xcd_cols_for(M, N, K, m_tiles, n_tiles);
  out[4] = parts;
  out[5] = t.bm; out[6] = t.bn; out[7] = t.sta; out[8] = t.stb; out[9] = t.lnx; out[10] = t.prod; out[11] = gemm_bwd_tile(cfg) ? 1 : 0;
  return UFND_OK;
}
